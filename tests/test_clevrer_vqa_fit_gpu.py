"""GPU: the training path of the Aloe reasoner (csrc/aloe_train.hip) against the float64 restatement of tests/aloe_fit_cases.py -- logits, losses,
recorded gates and every gradient at the smallest shapes that reach each edge of the kernels --, its determinism, the autograd node, the
reference's own gradients, `clevrer_vqa.fit` on a planted set and `clevrer_vqa.evaluate`.  Bar: the project's DEVICE_BAR (1e-3 relative, max |delta|
/ max |ref| per tensor); the measured figures are printed."""
import numpy as np
import pytest
import torch

import aloe_fit_cases as fc
import clevrer_vqa_cases as cases

pytestmark = pytest.mark.gpu
BAR = fc.DEVICE_BAR


def module_of(cfg, sd, dev):
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel
    tm = CLEVRERTransformerModel(*[dict(c) for c in cfg])
    tm.load_state_dict({k: v.clone() for k, v in sd.items()})
    return tm.to(dev)


def device_slots(tc, dev):
    s = torch.from_numpy(np.asarray(tc['slots']))
    if not tc.get('strided'):
        return s.to(dev)
    V, T_all, N, C = s.shape                         # the slots as a view of a wider table with NaN between the frames
    wide = torch.full((V, T_all, N + 1, C), float('nan'), device=dev)
    wide[:, :, :N] = s.to(dev)
    return wide[:, :, :N]


def batch_of(tc, dev):
    idx = lambda v: None if v is None else torch.as_tensor(np.asarray(v), device=dev)  # noqa: E731
    return dict(tokens=torch.from_numpy(tc['tokens']).to(dev), pad_mask=torch.from_numpy(tc['pad']).to(dev), B1=tc['B1'], video_index=idx(tc['video_index']),
                start=idx(tc['start']), frame_offset=tc['frame_offset'], num_frames=tc['T'])


def run_device(tc, dev, seed=None, want_gates=True, tm=None):
    """-> dict(cls_logits, mc_logits, losses, flat gradient buffer (entered full of NaN), gates, head_gates) as numpy"""
    from slotformer_amd import ops, train
    tm = module_of(tc['cfg'], tc['sd'], dev) if tm is None else tm
    slots = device_slots(tc, dev)
    batch = batch_of(tc, dev)
    seed = tc['seed'] if seed is None else seed
    desc, keep = train.aloe_model(tm, slots.shape[2], tc['T'], tc['tokens'].shape[1])
    cls_logits, mc_logits, ws, gates, head_gates = ops.aloe_train_fwd(desc, slots, batch, p=tc['p'], seed=seed, want_gates=want_gates)
    losses, g_cls, g_mc = ops.aloe_score_grad(cls_logits, tc['cls_label'], mc_logits, tc['mc_label'], tc['w_cls'], tc['w_mc'])
    n = sum(k for _, k in ops._aloe_layout_of(desc))
    flat = torch.full((n, ), float('nan'), device=dev)
    ops.aloe_train_bwd(desc, slots, batch, g_cls, g_mc, ws, p=tc['p'], seed=seed, out=flat)
    del keep
    cpu = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(cls_logits=cpu(cls_logits), mc_logits=cpu(mc_logits), losses=cpu(losses), flat=cpu(flat), gates=cpu(gates), head_gates=cpu(head_gates),
                g_cls=g_cls, g_mc=g_mc)


def compare(tc, got, label):
    """the device's run of `tc` against float64: logits and gates against float64's own run, losses and gradients against float64 on the device's
    gate pattern -> the worst relative error"""
    own = fc.loss_and_grads64(tc)
    errs = {'cls_logits': fc.rel_err(got['cls_logits'], own['cls_logits']), 'mc_logits': fc.rel_err(got['mc_logits'], own['mc_logits'])}
    B, L = own['live'].shape
    for i, ok in enumerate(fc.clear_of_band(own['pre'], own['live'])):
        mine = got['gates'][i].reshape(B, L, -1) if i < len(own['pre']) - 1 else got['head_gates']
        want = own['pre'][i].numpy() > 0
        assert np.array_equal(mine.astype(bool)[ok], want[ok]), (label, 'gates of layer / head', i)
    ref = fc.loss_and_grads64(tc, gates=got['gates'], head_gates=got['head_gates'])
    for k, (mine, want) in enumerate(zip(got['losses'], ref['losses'])):
        errs[f'loss{k}'] = abs(float(mine) - want) / abs(want) if want else abs(float(mine))
    assert np.isfinite(got['flat']).all(), (label, 'a gradient element was left unwritten or is not finite')
    grads = fc.split_flat(got['flat'], tc['cfg'], tc['sd'])
    for k in fc.grad_keys(tc['cfg']):
        errs[k] = fc.rel_err(grads[k], ref['grads'][k])
    worst = max(errs, key=errs.get)
    print(f'{label}: worst relative error {errs[worst]:.2e} ({worst}); logits {errs["cls_logits"]:.2e} / {errs["mc_logits"]:.2e}')
    for k, e in errs.items():
        assert e < BAR, (label, k, e)
    return errs[worst]


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
def test_forward_and_every_gradient_against_float64(dev, case):
    tc = fc.train_case(case)
    compare(tc, run_device(tc, dev), case['name'])


def test_loss_weights_scale_the_gradient(dev):
    tc = fc.train_case(fc.CASES[0], w_cls=0.5, w_mc=2.0)
    compare(tc, run_device(tc, dev), 'tiny-L6 with loss weights 0.5 / 2')


def test_equal_inputs_and_seed_give_equal_bits(dev):
    for case in (fc.CASES[7], fc.CASES[0]):      # p = 0.1 and p = 0
        tc = fc.train_case(case)
        a, b, c = run_device(tc, dev), run_device(tc, dev), run_device(tc, dev, seed=tc['seed'] + 1)
        for k in ('cls_logits', 'mc_logits', 'flat', 'gates'):
            assert np.array_equal(a[k], b[k]), (case['name'], k)
        same = np.array_equal(a['flat'], c['flat']) and np.array_equal(a['cls_logits'], c['cls_logits'])
        assert same == (tc['p'] == 0), case['name']


def test_training_forward_without_dropout_agrees_with_answer(dev):
    tc = fc.train_case(dict(fc.CASES[4], p=0.0))
    tm = module_of(tc['cfg'], tc['sd'], dev).eval()
    got = run_device(tc, dev, tm=tm)
    slots, b = device_slots(tc, dev), batch_of(tc, dev)
    B1 = tc['B1']
    for mc, lo, hi, key in ((False, 0, B1, 'cls_logits'), (True, B1, len(tc['tokens']), 'mc_logits')):
        want, _ = tm.answer(slots, b['tokens'][lo:hi], b['pad_mask'][lo:hi], mc, video_index=torch.arange(lo, hi, device=dev), num_frames=tc['T'])
        err = fc.rel_err(got[key].reshape(-1), want.cpu().numpy().reshape(-1))
        print(key, 'training forward at p = 0 vs answer():', err)
        assert err < BAR


def test_autograd_node_leaves_the_bits_of_the_direct_call(dev):
    from slotformer_amd import train
    tc = fc.train_case(fc.CASES[7])
    direct = run_device(tc, dev)
    tm = module_of(tc['cfg'], tc['sd'], dev).train()
    slots, batch = device_slots(tc, dev), batch_of(tc, dev)
    cls_logits, mc_logits = train.aloe_with_grad(tm, slots, batch, p=tc['p'], seed=tc['seed'])
    loss, parts = train.aloe_loss(cls_logits, mc_logits, torch.as_tensor(tc['cls_label'], device=dev), torch.as_tensor(tc['mc_label'], device=dev))
    loss.backward()
    assert np.array_equal(cls_logits.detach().cpu().numpy(), direct['cls_logits']) and np.array_equal(parts.cpu().numpy(), direct['losses'])
    flat = torch.cat([p.grad.reshape(-1) for p in train.aloe_parameters(tm)]).cpu().numpy()
    assert np.array_equal(flat, direct['flat'])
    # default p: the layers' own in train(), 0 in eval(); grad_out: the bucket gets the gradients, .grad stays None
    tm2 = module_of(tc['cfg'], tc['sd'], dev).train()
    bucket = torch.full((flat.size, ), float('nan'), device=dev)
    a, b = train.aloe_with_grad(tm2, slots, batch, seed=tc['seed'], grad_out=bucket)
    train.aloe_loss(a, b, torch.as_tensor(tc['cls_label'], device=dev), torch.as_tensor(tc['mc_label'], device=dev))[0].backward()
    assert np.array_equal(bucket.cpu().numpy(), direct['flat']) and all(p.grad is None for p in tm2.parameters())
    quiet = train.aloe_with_grad(tm2.eval(), slots, batch)[0]
    assert not np.array_equal(quiet.detach().cpu().numpy(), direct['cls_logits'])
    # the node keeps its descriptor in the module's plan cache: a module that went through it still copies and pickles, and the copy works
    import copy
    import pickle
    from slotformer_amd import plans
    assert 'aloe_train_model' in tm2.__dict__[plans._ATTR]
    twin = copy.deepcopy(tm2).train()
    pickle.loads(pickle.dumps(tm2))
    a2, _ = train.aloe_with_grad(twin, slots, batch, p=tc['p'], seed=tc['seed'])
    assert np.array_equal(a2.detach().cpu().numpy(), direct['cls_logits'])
    plans.invalidate(tm2)
    assert plans._ATTR not in tm2.__dict__


def test_reference_gradient_fixture(dev):
    tc = fc.fixture_train_case()
    got = run_device(tc, dev)
    worst = fc.check_against_golden(fc.split_flat(got['flat'], tc['cfg'], tc['sd']), [float(v) for v in got['losses']], BAR)
    g = np.load(fc.GOLDEN)
    print('device vs the reference fixture: worst gradient error', worst, 'logits', fc.rel_err(got['cls_logits'], g['cls_logits']),
          fc.rel_err(got['mc_logits'], g['mc_logits']))
    assert fc.rel_err(got['cls_logits'], g['cls_logits']) < BAR and fc.rel_err(got['mc_logits'], g['mc_logits']) < BAR


def fit_run(dev, seed):
    from slotformer_amd import clevrer_vqa
    from slotformer_amd.clevrer_vqa.models import CLEVRERAloe
    cfg, sd, slots, q = fc.fit_case()
    f = fc.FIT
    model = CLEVRERAloe(module_of(cfg, sd, dev))
    table = torch.from_numpy(slots).to(dev)
    losses = clevrer_vqa.fit(model, table, q, f['epochs'], batch_size=f['batch_size'], lr=f['lr'], seed=seed)
    return model, table, q, losses.cpu().numpy()


def test_fit_learns_the_planted_set(dev):
    from slotformer_amd import clevrer_vqa
    model, table, q, losses = fit_run(dev, fc.FIT['seed'])
    total = losses.sum(-1)
    print('fit: epoch losses (CE + BCE) first', total[0], 'last', total[-1], 'ratio', total[-1] / total[0])
    assert losses.shape == (fc.FIT['epochs'], 2) and np.isfinite(losses).all()
    assert total[-1] < 0.5 * total[0]
    sd = {k: v.detach().cpu() for k, v in model.transformer_model.state_dict().items()}
    assert all(torch.isfinite(v).all() for v in sd.values()) and not model.training
    # one seed, one result, bit for bit; another seed, another result
    again, _, _, losses2 = fit_run(dev, fc.FIT['seed'])
    assert np.array_equal(losses, losses2)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in again.transformer_model.state_dict().items())
    assert not np.array_equal(losses, fit_run(dev, fc.FIT['seed'] + 1)[3])
    # answer() afterwards sees the trained weights (and a fresh text table)
    cfg = fc.fit_case()[0]
    flag = q['mc_flag']
    for mc, tok, pad, vidx in ((False, q['cls_q_tokens'], q['cls_q_pad_mask'], q['cls_video_index']),
                               (True, q['mc_q_tokens'], q['mc_q_pad_mask'], q['mc_video_index'][flag])):
        want = cases.forward64(sd, cfg, table.cpu().numpy(), tok, pad, mc, video_index=vidx)
        got, _ = model.transformer_model.answer(table, torch.from_numpy(tok).to(dev), torch.from_numpy(pad).to(dev), mc,
                                                video_index=torch.from_numpy(vidx).to(dev))
        err = fc.rel_err(got.cpu().numpy().reshape(want.shape), want)
        print('answer() after fit vs float64 of the trained weights:', err)
        assert err < BAR
    ev = clevrer_vqa.evaluate(model, table, q, batch_size=7)
    print('evaluate after fit:', ev)
    assert ev['descriptive_bs'] == 32 and ev['multiple-choice_bs'] == 16


def test_evaluate_equals_the_numpy_reference(dev):
    from slotformer_amd import clevrer_vqa
    from slotformer_amd.clevrer_vqa.models import CLEVRERAloe
    hc = cases.harness_case()
    cfg, sd, slots, q, T = hc
    cls64, mc64 = cases.harness64(hc)
    for logits, mc in ((cls64, False), (mc64, True)):
        margin, bar = cases.clearance(logits, mc)
        assert margin > bar, (margin, bar)
    cls_label = np.argmax(cls64, -1)
    cls_label[[1, 3]] = (cls_label[[1, 3]] + 1) % 9                     # three of five right
    mc_label = (mc64 > 0).astype(np.float32)
    mc_label[[3, 5]] = 1 - mc_label[[3, 5]]                             # questions 1 and 2 wrong
    q = dict(q, cls_label=cls_label, mc_label=mc_label, mc_subtype=np.array([1, 2, 3, 3]))
    want, _ = cases.eval_reference(cls64, cls_label, mc64, mc_label, q['mc_flag'], q['mc_subtype'])
    model = CLEVRERAloe(module_of(cfg, sd, dev)).eval()
    got = clevrer_vqa.evaluate(model, torch.from_numpy(slots).to(dev), q, batch_size=3)
    assert set(got) == set(want) and len(got) == 10
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k
