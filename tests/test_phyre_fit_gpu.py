"""GPU: the training path of the PHYRE readout (csrc/phyre_readout_train.hip: one launch per layer in each direction) against the float64
restatement of tests/phyre_fit_cases.py -- logits, the recorded ReLU gates outside the band, every gradient on the device's gate pattern --,
determinism, written-not-accumulated buffers, the eval-mode forward at p = 0, the REFERENCE's gradients (tests/golden/phyre_readout_grads.npz),
the autograd node, `phyre_planning.fit` on a planted set and `phyre_planning.evaluate`.  The bound is the project's 1e-3 relative bar
(measured: profiles/phyre_fit.md)."""
import numpy as np
import pytest
import torch

import phyre_fit_cases as fc
import phyre_readout_cases as cases

pytestmark = pytest.mark.gpu
BAR = fc.DEVICE_BAR


@pytest.fixture(autouse=True)
def split_bf16():
    """the layers exist in split-bf16 only (the process default) -- restored afterwards"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(1)
    yield lib
    lib.sf_set_precision(old)


def rel_err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def readout_on(dev, rd, sd):
    from slotformer_amd.phyre_planning.models import PHYREReadout
    m = PHYREReadout(rd)
    m.load_state_dict(sd)
    return m.to(dev)


def slots_on(dev, tc, strided=False):
    s = torch.from_numpy(tc['slots']).to(dev)
    if strided:
        # every second video of a buffer that holds two slot sets per frame: video and frame strides larger than the extents, NaN in between
        V, T_all, N, C = s.shape
        big = torch.full((2 * V, T_all, 2, N, C), float('nan'), device=dev)
        big[::2, :, 0] = s
        s = big[::2, :, 0]
        assert not s.is_contiguous() and s.stride(1) == 2 * N * C
    return s


def device_run(dev, tc, strided=False, seed=None, p=None, want_gates=True):
    """forward + backward of a case through ops -> dict(logits, gates, head_gates, flat: numpy); g = d mean-BCE / d logit from the score kernel.
    The gradient buffer is handed over full of NaN: the call writes, it does not accumulate."""
    from slotformer_amd import ops, train
    m = readout_on(dev, tc['rd'], tc['sd'])
    model, keep = train.phyre_readout_model(m)
    s = slots_on(dev, tc, strided)
    vidx = None if tc['video_index'] is None else torch.tensor(tc['video_index'], dtype=torch.int32, device=dev)
    seed = tc['seed'] if seed is None else seed
    p = tc['p'] if p is None else p
    logits, ws, gates, head_gates = ops.phyre_readout_train_fwd(model, s, tc['table'], video_index=vidx, p=p, seed=seed, want_gates=want_gates)
    loss, g, _, _ = ops.physion_readout_score(logits, torch.from_numpy(tc['labels']).to(dev))
    n = sum(k for _, k in ops.phyre_grad_layout(tc['rd']['slot_size'], len(tc['table']), tc['rd']['num_layers'], tc['learnable_pe']))
    flat = torch.full((n, ), float('nan'), dtype=torch.float32, device=dev)
    out = ops.phyre_readout_train_bwd(model, s, tc['table'], g, ws, video_index=vidx, p=p, seed=seed, learnable_pe=tc['learnable_pe'], out=flat)
    torch.cuda.synchronize()
    assert out is flat
    del keep
    return dict(logits=logits.cpu().numpy(), gates=None if gates is None else gates.cpu(), head_gates=None if head_gates is None else head_gates.cpu(),
                flat=flat.cpu().numpy(), loss=float(loss[0]), g=g, model=m)


_RUNS = {}


def case_run(dev, case):
    """one device run and one float64 run (its own gates) per case, shared by the tests below and left unchanged"""
    if case['name'] not in _RUNS:
        tc = fc.train_case(case)
        _RUNS[case['name']] = (tc, device_run(dev, tc, strided=case.get('strided', False)), fc.loss_and_grads64(tc))
    return _RUNS[case['name']]


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
def test_logits_gates_and_gradients_vs_float64(dev, case):
    tc, run, (loss64, logits64, _, pre) = case_run(dev, case)
    rd = tc['rd']
    B, L, nl = case['B'], 1 + case['T'] * case['N'], case['nl']
    # 1. the forward, against float64 with float64's own gates
    e_fwd = rel_err(run['logits'], logits64)
    assert run['logits'].shape == (B, ) and e_fwd < BAR
    assert abs(run['loss'] - loss64) < BAR * max(1.0, abs(loss64))
    # 2. the recorded gates: equal to float64's wherever |h64| >= BAR max|h64| of the layer
    dev_gates = [run['gates'][i].reshape(B, L, 512) for i in range(nl)] + [run['head_gates']]
    assert run['gates'].shape == (nl, B * L, 512) and run['head_gates'].shape == (B, 128)
    flipped = 0
    for gd, h, clear in zip(dev_gates, pre, fc.clear_of_band(pre)):
        assert set(np.unique(gd.numpy()).tolist()) <= {0, 1}
        same = gd.bool() == (h > 0)
        assert bool(same[clear].all())
        flipped += int((~same).sum())
    # 3. the gradients, against float64 on the DEVICE's gate pattern
    _, _, grads64, _ = fc.loss_and_grads64(tc, gates=dev_gates[:nl], head_gates=dev_gates[nl])
    mine = fc.split_flat(run['flat'], rd, tc['learnable_pe'], tc['sd'])
    worst, worst_key = 0.0, None
    for k, ref in grads64.items():
        e = rel_err(mine[k], ref)
        if not e <= worst:
            worst, worst_key = e, k
    print(f"{case['name']}: B {B} L {L} C {case['C']} layers {nl} p {case['p']}: logits {e_fwd:.2e}, gates flipped inside the band {flipped}, "
          f"worst gradient {worst:.2e} ({worst_key})")
    for k, ref in grads64.items():
        assert rel_err(mine[k], ref) < BAR, k   # NaN (an unwritten element) fails it


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
def test_equal_inputs_equal_bits_and_written_not_accumulated(dev, case):
    tc, run, _ = case_run(dev, case)
    assert np.isfinite(run['flat']).all() and np.isfinite(run['logits']).all()   # the buffer went in full of NaN
    again = device_run(dev, tc, strided=case.get('strided', False))
    assert np.array_equal(again['logits'], run['logits']) and np.array_equal(again['flat'], run['flat'])
    assert torch.equal(again['gates'], run['gates']) and torch.equal(again['head_gates'], run['head_gates'])
    other = device_run(dev, tc, strided=case.get('strided', False), seed=tc['seed'] + 1)
    if case['p'] > 0:
        assert not np.array_equal(other['logits'], run['logits']) and not np.array_equal(other['flat'], run['flat'])
    else:
        assert np.array_equal(other['logits'], run['logits']) and np.array_equal(other['flat'], run['flat'])


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
@torch.no_grad()
def test_training_forward_without_dropout_is_the_eval_forward(dev, case):
    tc = fc.train_case(case)
    run = device_run(dev, tc, strided=case.get('strided', False), p=0.0, want_gates=False)
    assert run['gates'] is None and run['head_gates'] is None
    m = run['model'].eval()
    vidx = None if tc['video_index'] is None else torch.tensor(tc['video_index'], dtype=torch.int32, device=dev)
    ev = m.logits_of(slots_on(dev, tc, case.get('strided', False)), sel=tc['table'], video_index=vidx)[0]
    e = rel_err(run['logits'], ev.cpu().numpy())
    print(f"{case['name']}: training forward at p = 0 vs logits_of: {e:.2e}")
    assert e < BAR


def test_reference_gradients(dev):
    """the REFERENCE's own PHYREReadout, eval(), calc_train_loss(...).backward() -- tests/golden/phyre_readout_grads.npz"""
    tc = fc.fixture_train_case()
    run = device_run(dev, tc, p=0.0)
    worst = fc.check_against_golden(fc.split_flat(run['flat'], tc['rd'], False, tc['sd']), run['loss'], BAR)
    print(f'reference gradient fixture: worst relative error {worst:.2e}')


def test_autograd_node_leaves_the_bits_of_the_backward_call(dev):
    from slotformer_amd import train
    case = fc.CASES[1]
    tc, run, _ = case_run(dev, case)
    labels = torch.from_numpy(tc['labels']).to(dev)
    s = slots_on(dev, tc)
    m = readout_on(dev, tc['rd'], tc['sd']).train()
    logits = train.phyre_readout_with_grad(m, s, sel=tc['table'], seed=tc['seed'])   # (p: the layers' own 0.1, the module is in train())
    assert logits.requires_grad and np.array_equal(logits.detach().cpu().numpy(), run['logits'])
    loss = train.readout_loss(logits, labels)
    loss.backward()
    params = train.phyre_readout_parameters(m)
    got = torch.cat([p.grad.reshape(-1) for p in params]).cpu().numpy()
    assert np.array_equal(got, run['flat'])
    # eval(): p defaults to 0; p= overrides
    m.eval()
    l0 = train.phyre_readout_with_grad(m, s, sel=tc['table'])
    l1 = train.phyre_readout_with_grad(m, s, sel=tc['table'], p=0.1, seed=tc['seed'])
    assert not np.array_equal(l0.detach().cpu().numpy(), run['logits']) and np.array_equal(l1.detach().cpu().numpy(), run['logits'])
    # grad_out=: the same bits in the caller's bucket, .grad left alone
    m2 = readout_on(dev, tc['rd'], tc['sd']).train()
    bucket = torch.full((got.size, ), float('nan'), dtype=torch.float32, device=dev)
    train.readout_loss(train.phyre_readout_with_grad(m2, s, sel=tc['table'], seed=tc['seed'], grad_out=bucket), labels).backward()
    assert np.array_equal(bucket.cpu().numpy(), run['flat'])
    assert all(p.grad is None for p in train.phyre_readout_parameters(m2))


def fit_run(dev, seed):
    from slotformer_amd import phyre_planning
    rd, sd, slots, labels = fc.fit_case()
    m = readout_on(dev, rd, sd)
    f = fc.FIT
    s, y = torch.from_numpy(slots).to(dev), torch.from_numpy(labels).to(dev)
    losses = phyre_planning.fit(m, s, y, f['epochs'], batch_size=f['batch_size'], lr=f['lr'], seed=seed, warmup_steps_pct=f['warmup'])
    torch.cuda.synchronize()
    return m, s, y, losses.cpu().numpy(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_fit_on_the_planted_set(dev):
    from slotformer_amd import phyre_planning
    rd, sd, slots, labels = fc.fit_case()
    m, s, y, losses, state = fit_run(dev, fc.FIT['seed'])
    print('device fit: losses', ['%.4f' % v for v in losses])
    assert losses.shape == (fc.FIT['epochs'], ) and np.isfinite(losses).all()
    assert losses[-1] < 0.1 * losses[0] and losses[len(losses) // 2] < losses[0]
    assert not m.training
    # the next logits_of sees the trained weights: the plan cache was dropped
    ref, _ = fc.forward64({k: v.double() for k, v in state.items()}, rd, slots, rd['sel_slots'])
    e = rel_err(m.logits_of(s)[0], ref.numpy())
    print(f'eval forward of the trained module vs float64 of its state dict: {e:.2e}')
    assert e < BAR
    ev = phyre_planning.evaluate(m, s, y, batch_size=24)
    assert ev['acc_0.50'] == 1.0 and np.isfinite(ev['loss']) and list(ev) == ['loss'] + [f'acc_{t:.2f}' for t in cases.EVAL_THRESHS]
    # one seed, one result; another seed, another
    _, _, _, losses2, state2 = fit_run(dev, fc.FIT['seed'])
    assert np.array_equal(losses, losses2) and all(torch.equal(state[k], state2[k]) for k in state)
    _, _, _, losses3, state3 = fit_run(dev, fc.FIT['seed'] + 1)
    assert not np.array_equal(losses, losses3) and any(not torch.equal(state[k], state3[k]) for k in state)


@torch.no_grad()
def test_evaluate_counts(dev):
    """loss and the five counts over a set cut into ragged batches, against float64 on a case whose confidences stay clear of the thresholds"""
    from slotformer_amd import phyre_planning
    rd = cases.readout_dict(4, 32, (0, 1), 2)
    V = 37
    for seed in range(600, 620):   # (seeded: the first weights whose confidences clear every threshold by the margin)
        sd = cases.seeded_weights(rd, seed)
        slots = cases.seeded_slots(seed + 1, V, 2, 4, 32)
        ref = cases.forward64(sd, rd, slots)
        if cases.threshold_clearance(ref) > cases.THRESH_MARGIN(ref):
            break
    else:
        raise AssertionError('no seeded case clears the thresholds')
    labels = (np.random.default_rng(seed + 2).uniform(size=V) > 0.5).astype(np.float32)
    m = readout_on(dev, rd, sd).eval()
    ev = phyre_planning.evaluate(m, torch.from_numpy(slots).to(dev), torch.from_numpy(labels).to(dev), batch_size=16)
    for t in cases.EVAL_THRESHS:
        assert round(ev[f'acc_{t:.2f}'] * V) == int(cases.hits64(ref, labels, t).sum()), t
    assert abs(ev['loss'] - cases.loss64(ref, labels)) < BAR * cases.loss64(ref, labels)
    assert not m.training
