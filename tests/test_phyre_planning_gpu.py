"""GPU: PHYRE planning on the device (csrc/phyre_readout.hip + the token-stationary layers of csrc/layer_tok128.hip) -- the readout's forward
against the float64 restatement of tests/phyre_readout_cases.py at every shape edge and against the REFERENCE's fixture, calc_eval_loss,
SingleStepSlotFormer with the classifier attached, harness.phyre_plan against the module-call path, and the AUCCESS ranks against the reference's
loop.  The bound on the logits is the project's 1e-3 relative bar (measured: profiles/phyre_planning.md)."""
import copy
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import golden_util as gu
import phyre_readout_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'phyre_readout.npz')


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
    return m.eval().to(dev)


@pytest.mark.parametrize('case', cases.FORWARD_CASES, ids=lambda c: c['name'])
@torch.no_grad()
def test_forward_vs_float64(dev, case):
    rd, sd, slots, table = cases.forward_case(case)
    ref = cases.forward64(sd, rd, slots, table, case.get('video_index'))
    m = readout_on(dev, rd, sd)
    s = torch.from_numpy(slots).to(dev)
    if case.get('strided'):
        # every second video of a buffer that holds two slot sets per frame: video and frame strides larger than the extents, NaN in between
        V, T_all, N, C = s.shape
        big = torch.full((2 * V, T_all, 2, N, C), float('nan'), device=dev)
        big[::2, :, 0] = s
        s = big[::2, :, 0]
        assert not s.is_contiguous() and s.stride(1) == 2 * N * C
    vidx = case.get('video_index')
    vidx = None if vidx is None else torch.tensor(vidx, dtype=torch.int32, device=dev)
    logits, conf = m.logits_of(s, sel=table, video_index=vidx, want_conf=True)
    torch.cuda.synchronize()
    assert logits.shape == (case['B'], ) and logits.dtype == torch.float32
    e = rel_err(logits, ref)
    print(f"{case['name']}: B {case['B']} L {1 + case['T'] * case['N']} C {case['C']} layers {case['nl']}: rel err vs float64 {e:.2e}")
    assert e < cases.DEVICE_BAR      # NaN (an unwritten row) fails it
    assert np.abs(conf.cpu().numpy() - cases.sigmoid64(logits.cpu().numpy())).max() < 1e-6
    # through forward(): a model whose sel_slots is the table (frame numbers only) gives the same bits
    if min(table) >= 0:
        data = {'slots': s} if vidx is None else {'slots': s, 'video_index': vidx}
        assert torch.equal(m(data)['logits'], logits)
    # twice the same bits; a sequence does not depend on the others of the call
    again, _ = m.logits_of(s, sel=table, video_index=vidx)
    assert torch.equal(again, logits)
    if vidx is None and case['B'] >= 2:
        keep = case['B'] // 2
        alone, _ = m.logits_of(s, sel=table, video_index=torch.tensor([keep], dtype=torch.int32, device=dev))
        assert rel_err(alone, ref[keep:keep + 1]) < cases.DEVICE_BAR


@torch.no_grad()
def test_scatter_and_plan_cache(dev):
    """The head kernel writes the confidences into a caller's table; an index outside it is skipped.  A changed weight rebuilds the packed layers."""
    from slotformer_amd import engine
    case = cases.FORWARD_CASES[2]
    rd, sd, slots, table = cases.forward_case(case)
    m = readout_on(dev, rd, sd)
    s = torch.from_numpy(slots).to(dev)
    B = case['B']
    out = torch.full((2 * B + 1, ), -1.0, device=dev)
    index = torch.arange(B, dtype=torch.int32, device=dev) * 2 + 1
    index[B - 1] = 2 * B + 1   # one past the table
    logits, conf = m.logits_of(s, sel=table, want_conf=True, scatter_index=index, scatter_table=out)
    torch.cuda.synchronize()
    want = torch.full_like(out, -1.0)
    want[1:2 * B - 1:2] = conf[:B - 1]
    assert torch.equal(out, want)
    plan = engine.phyre_readout_plan(m)
    assert engine.phyre_readout_plan(m) is plan
    m.transformer_encoder.layers[1].linear1.weight.mul_(1.5)
    assert engine.phyre_readout_plan(m) is not plan
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2['transformer_encoder.layers.1.linear1.weight'] *= 1.5
    assert rel_err(m.logits_of(s, sel=table)[0], cases.forward64(sd2, rd, slots, table)) < cases.DEVICE_BAR


@torch.no_grad()
def test_reference_fixture_and_eval_loss(dev):
    g = np.load(GOLDEN)
    rd, sd, slots, labels = cases.fixture_case()
    m = readout_on(dev, rd, sd)
    data = {'slots': torch.from_numpy(slots).to(dev), 'label': torch.from_numpy(labels).to(dev)}
    out = m(data)
    e = rel_err(out['logits'], g['logits'])
    print(f'reference fixture: rel err {e:.2e}')
    assert e < cases.DEVICE_BAR
    ev = m.calc_eval_loss(data, out)
    assert list(ev) == ['vqa_loss'] + json.loads(str(g['acc_keys']))
    assert abs(float(ev['vqa_loss']) - float(g['vqa_loss'])) < cases.DEVICE_BAR * abs(float(g['vqa_loss']))
    assert np.array_equal(np.float32([float(ev[k]) for k in json.loads(str(g['acc_keys']))]), g['acc'])   # exact counts / B
    tr = m.calc_train_loss(data, out)
    assert list(tr) == ['vqa_loss'] and float(tr['vqa_loss']) == float(ev['vqa_loss'])
    # exact counts on a larger seeded case against the float64 confidences (no confidence lies near a threshold: tests/test_phyre_planning.py)
    case = next(c for c in cases.FORWARD_CASES if c['name'] == 'b23-n7-t3')
    rd, sd, slots, table = cases.forward_case(case)
    ref = cases.forward64(sd, rd, slots, table)
    lab = (cases.sigmoid64(ref) > np.median(cases.sigmoid64(ref))).astype(np.float32)
    lab[::3] = 1 - lab[::3]
    m = readout_on(dev, rd, sd)
    data = {'slots': torch.from_numpy(slots).to(dev), 'label': torch.from_numpy(lab).to(dev)}
    ev = m.calc_eval_loss(data, m(data))
    for t in cases.EVAL_THRESHS:
        assert round(float(ev[f'acc_{t:.2f}']) * case['B']) == int(cases.hits64(ref, lab, t).sum()), t
    assert abs(float(ev['vqa_loss']) - cases.loss64(ref, lab)) < cases.DEVICE_BAR * cases.loss64(ref, lab)


@torch.no_grad()
def test_training_mode_and_unsupported_use_on_the_device(dev):
    rd, sd, slots, _ = cases.fixture_case()
    m = readout_on(dev, rd, sd)
    s = torch.from_numpy(slots).to(dev)
    with pytest.raises(NotImplementedError, match='not built'):
        m.train()({'slots': s})
    m.eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m({'slots': s.cpu()})
    with pytest.raises(ValueError):
        m({'slots': s[:, :, :7]})
    with pytest.raises(IndexError):
        m({'slots': s[:, :3]})          # sel_slots [0, 3] on three frames


def _slotformer_c5(dev):
    from test_engine_gpu import build
    sf, _ = build(gu.C5_ROLL, gu.load_golden('roll_c5'), 205, dev, vp=True)
    return sf


@torch.no_grad()
def test_single_step_slotformer_with_the_classifier_attached(dev):
    """single_step_slotformer.py:119-129: logits = success_cls(cat(gt_slots, pred_slots))."""
    rd, sd, _, _ = cases.fixture_case()
    readout = readout_on(dev, rd, sd)
    sf = _slotformer_c5(dev)
    sf.success_cls, sf.use_cls_loss = readout, True
    sf.eval()
    vid_len = max(rd['sel_slots']) + 1
    sf.rollout_len = vid_len - sf.history_len
    slots = gu.seeded_normal((3, vid_len, 8, 128), 91).to(dev)   # (the frames behind the first are NOT zeros here: gt_slots must show)
    out = sf({'slots': slots})
    cat = torch.cat([out['gt_slots'], out['pred_slots']], 1)
    assert cat.shape == (3, 2 * (vid_len - 1), 8, 128)
    assert torch.equal(out['logits'], readout({'slots': cat})['logits'])
    assert rel_err(out['logits'], cases.forward64(sd, rd, cat.cpu().numpy())) < cases.DEVICE_BAR
    sf.use_cls_loss = False
    assert 'logits' not in sf({'slots': slots})


def _planning_models(dev):
    """The C5 pair (PHYRE SAVi + SingleStepSlotFormer) at the smallest resolution the encoder takes, 64 x 64."""
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    torch.manual_seed(77)
    scfg = gu.savi_cfg(64, 8, iters=2, kernel_mlp=True, pred='transformer', rnn=True, kld='none', dec_res=(8, 8))
    savi = bb(gu.ParamsView(scfg))
    path = os.path.join(tempfile.mkdtemp(), 'savi.pth')
    torch.save({'state_dict': savi.state_dict()}, path)
    rcfg = copy.deepcopy(gu.C5_ROLL)
    rcfg['resolution'] = (64, 64)
    rcfg['dec_dict'] = dict(scfg['dec_dict'], dec_ckp_path=path)
    sf = bv(gu.ParamsView(rcfg))
    savi.testing = True
    return savi.eval().to(dev), sf.eval().to(dev)


@pytest.mark.parametrize('batch_size', [128, 3])
@torch.no_grad()
def test_phyre_plan_vs_the_module_call_path(dev, batch_size):
    """Five first frames, one of them an INVALID action.  reference_indexing=True: savi -> pad -> SingleStepSlotFormer with the classifier
    attached -> sigmoid, as test_phyre_planning.py does it; False: the classifier on [slot0, predictions].  Both paths run the same kernels, in
    forms that each stay within 5e-5 of float64 on the slots, so the confidences may differ by a few 1e-5; the bound is a quarter of the
    project's bar on the logits (sigmoid' <= 1/4), 2.5e-4."""
    from slotformer_amd import harness, phyre_planning
    rd, sd, _, _ = cases.fixture_case()
    readout = readout_on(dev, rd, sd)
    savi, sf = _planning_models(dev)
    frames = gu.seeded_img(5, 1, 64, seed=4321)
    statuses = np.array([phyre_planning.NOT_SOLVED, 1, phyre_planning.INVALID_INPUT, 2, phyre_planning.NOT_SOLVED])
    valid = torch.from_numpy(statuses != 0)
    vid_len = max(rd['sel_slots']) + 1
    # the module-call path on the valid actions
    sf.success_cls, sf.use_cls_loss = readout, True
    out = harness.encode_then_rollout(savi, sf, frames[valid], vid_len)
    want_ref = torch.sigmoid(out['logits']).cpu()
    slot0 = savi({'img': frames[valid].to(dev)})['post_slots']
    want_trained = torch.sigmoid(readout({'slots': torch.cat([slot0, out['pred_slots']], 1)})['logits']).cpu()
    assert (want_ref - want_trained).abs().max() > 1e-3     # (the two index rules feed the classifier different frames)
    try:
        for reference_indexing, want in ((True, want_ref), (False, want_trained)):
            conf = harness.phyre_plan(savi, sf, readout, frames, statuses, batch_size=batch_size, reference_indexing=reference_indexing)
            assert conf.shape == (5, ) and conf.dtype == torch.float32 and conf.device.type == 'cpu'
            assert conf[2] == -1.0
            d = (conf[valid] - want).abs().max().item()
            print(f'phyre_plan batch_size {batch_size} reference_indexing {reference_indexing}: max |conf - module path| {d:.2e}')
            assert d < 2.5e-4
            on_dev = harness.phyre_plan(savi, sf, readout, frames.to(dev), statuses, batch_size=batch_size,
                                        reference_indexing=reference_indexing, to_host=False)
            assert on_dev.is_cuda and (on_dev.cpu() - conf).abs().max() < 2.5e-4 and on_dev[2] == -1.0
        every = harness.phyre_plan(savi, sf, readout, frames, batch_size=batch_size)   # no statuses: every action is valid
        assert (every > 0).all() and (every[valid] - want_ref).abs().max() < 2.5e-4
    finally:
        harness.release_pipelines()


@torch.no_grad()
def test_auccess_ranks_and_metric(dev):
    from slotformer_amd import ops, phyre_planning
    for name, (conf, status) in cases.auccess_cases().items():
        ranks = ops.phyre_auccess_ranks(torch.from_numpy(conf).to(dev), torch.from_numpy(status).to(dev))
        assert ranks.dtype == torch.int32 and ranks.shape == (conf.shape[0], )
        got = phyre_planning.auccess(conf, status)
        assert np.array_equal(got['first_rank'], ranks.cpu().numpy())
        if name == 'tie':
            assert ranks.tolist() == [cases.AUCCESS_EXPECTED_TIE_RANK]   # a solved action wins ties
            continue
        ref_auccess, ref_rate, _, ref_first = cases.auccess_reference(conf, status)
        assert np.array_equal(ranks.cpu().numpy(), ref_first), name
        assert np.array_equal(got['success_rate'], ref_rate) and got['auccess'] == pytest.approx(ref_auccess, rel=1e-12, abs=1e-12)
    conf, status = cases.auccess_cases()['three-tasks']
    ranks = ops.phyre_auccess_ranks(torch.from_numpy(conf).to(dev), torch.from_numpy(status).to(dev)).tolist()
    assert ranks[1] == 257 and 0 < ranks[0] < 257 and 3 <= ranks[2] <= 5
    conf, status = cases.auccess_cases()['first-and-last']
    ranks = ops.phyre_auccess_ranks(torch.from_numpy(conf).to(dev), torch.from_numpy(status).to(dev)).tolist()
    assert ranks == [0, 150 - 3 - 1]
    # a row shorter than 100 actions without a solved action never succeeds
    short = phyre_planning.auccess(np.linspace(0, 1, 7, dtype=np.float32)[None], np.full((1, 7), -1, np.int32))
    assert short['first_rank'].tolist() == [7] and short['auccess'] == 0.0
    # statuses as the reference's float arrays, tensors on the device
    conf, status = cases.auccess_cases()['three-tasks']
    again = phyre_planning.auccess(torch.from_numpy(conf).to(dev), torch.from_numpy(status.astype(np.float64)).to(dev))
    assert again['auccess'] == phyre_planning.auccess(conf, status)['auccess']
