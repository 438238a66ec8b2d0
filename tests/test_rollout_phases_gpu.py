"""GPU: the rollout at a frame offset in one call (sf_rollout_phases_f32 / engine.rollout_phases / harness.rollout_video_slots(one_call=True))
against the untouched engine.rollout run once per phase on gathered copies -- what rollout_video_slots does by default.

Bounds: bit for bit where the header promises batch-independent bits (sf_rollout_is_fused and layer_tok off); elsewhere 2e-5 of the largest
reference value, the bound between kernel forms of tests/test_pipeline_gpu.py (`_close`).  The shapes are the smallest that still cross the
boundary kernel's 32-row tiles with video edges inside them."""
import ctypes as C

import pytest
import torch

import golden_util as gu
from test_engine_gpu import build, rel_err
from test_pipeline_gpu import _close

pytestmark = pytest.mark.gpu

CANARY = -777.25


def _rollouter(dev, cfg, seed):
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(seed)
    return SlotRollouter(**cfg['rollout_dict']).eval().to(dev)


_cache = {}


def rollouter(dev, name):
    if name not in _cache:
        cfg, seed = {'c2': (gu.C2_ROLL, 11), 'c4_ref': (gu.C4_ROLL_REF, 12), 'c1': (gu.C1_ROLL, 13), 'c4': (gu.C4_ROLL, 14)}[name]
        _cache[name] = (_rollouter(dev, cfg, seed), cfg['rollout_dict'])
    return _cache[name]


def setup_case(dev, name, B, f, obs, pred_len, seed):
    """-> the rollouter, a buffer [B, T_total, N, C] with one canary frame behind the written ones (and canaries before `first`), its sizes"""
    roll, rd = rollouter(dev, name)
    hist, N, Cs = rd['history_len'], rd['num_slots'], rd['slot_size']
    S = -(-pred_len // f)
    T_total = obs + S * f + 1
    first = obs - hist * f
    buf = gu.seeded_normal((B, T_total, N, Cs), seed).to(dev)
    buf[:, :first] = CANARY
    buf[:, obs:] = CANARY
    return roll, buf, hist, S, first


def per_phase_reference(roll, buf, hist, f, obs, S, opts=None):
    """engine.rollout on a gathered copy of every phase (rollout_clevrer_slots.py:40-59), written back where the frames belong"""
    from slotformer_amd import engine
    ref = buf.clone()
    first = obs - hist * f
    for p in range(f):
        sub = torch.empty(buf.shape[0], hist + S, *buf.shape[2:], device=buf.device)
        sub[:, :hist] = buf[:, first + p:obs:f]
        engine.rollout(roll, sub, hist, S, ws_slot='ref', opts=opts)
        ref[:, obs + p:obs + S * f:f] = sub[:, hist:]
    return ref


def exact(roll, opts):
    from slotformer_amd import _lib, engine
    fused = _lib.lib().sf_rollout_is_fused(C.byref(engine.rollouter_plan(roll).struct)) == 1
    return fused and not (opts or {}).get('layer_tok')


def check_case(dev, name, B, f, obs, pred_len, seed, opts=None):
    from slotformer_amd import engine
    roll, buf, hist, S, first = setup_case(dev, name, B, f, obs, pred_len, seed)
    with torch.no_grad():
        ref = per_phase_reference(roll, buf, hist, f, obs, S, opts)
        out = buf.clone()
        assert engine.rollout_phases(roll, out, obs, pred_len, f, opts=opts) is out
        torch.cuda.synchronize()
    # never written: frames before `first`, the burn-in frames, the frame behind the last written one
    assert torch.equal(out[:, :obs], buf[:, :obs])
    assert torch.equal(out[:, obs + S * f:], buf[:, obs + S * f:])
    assert (out[:, obs + S * f:] == CANARY).all() and (out[:, :first] == CANARY).all()
    # written: every frame of [obs, obs + S f), the padded ones included
    assert torch.isfinite(out).all() and not (out[:, obs:obs + S * f] == CANARY).any()
    pred, rpred = out[:, obs:obs + S * f], ref[:, obs:obs + S * f]
    d = ((pred - rpred).abs().max() / rpred.abs().max()).item()
    print(f'{name} B {B} f {f} obs {obs} pred_len {pred_len} opts {opts}: one call vs one call per phase, max |d| / max |ref| = {d:.3e}')
    if exact(roll, opts):
        assert torch.equal(pred, rpred)
    else:
        assert _close(pred, rpred)
    return roll, buf, out


@pytest.mark.parametrize('opts', [None, {'seam': False}, {'attn_heads': 8}, {'attn_rows': 128, 'ffn_tile': 1}, {'attn_rows': 128, 'ffn_tile': 2},
                                  {'layer_tok': True}], ids=['default', 'noseam', 'heads8', 'rows128_tile1', 'rows128_tile2', 'tok'])
def test_c2_two_phases(dev, opts):
    """6 virtual videos x 7 slots = 42 rows: two 32-row boundary tiles with video edges inside them; S = 3, so one padded frame is written"""
    from slotformer_amd import _lib, engine
    roll, _, _ = check_case(dev, 'c2', 3, 2, 14, 5, 401, opts)
    st = engine.rollouter_plan(roll).struct
    o = engine.rollout_opts(opts)
    seam = _lib.lib().sf_rollout_uses_seam_opts(C.byref(st), 6, None if o is None else C.byref(o))
    assert seam == (1 if opts is None else 0)   # the default case is the one with seam launches
    if opts == {'layer_tok': True}:
        assert _lib.lib().sf_rollout_tok_layers(C.byref(st), 6, C.byref(o)) == st.num_layers - 1


def test_c2_three_phases_four_tiles(dev):
    check_case(dev, 'c2', 5, 3, 18, 6, 402)   # 15 virtual videos, 105 rows: four tiles


@pytest.mark.parametrize('tok', [False, True])
def test_long_window_three_phases(dev, tok):
    """C4_ROLL_REF (15 frames x 6 slots = 90 tokens, slot size 192): the long-window path, its window staged per step"""
    from slotformer_amd import _lib, engine
    roll, _, _ = check_case(dev, 'c4_ref', 2, 3, 45, 7, 403, {'layer_tok': tok})
    o = engine.rollout_opts({'layer_tok': tok})
    st = engine.rollouter_plan(roll).struct
    assert _lib.lib().sf_rollout_tok_layers(C.byref(st), 6, C.byref(o)) == (st.num_layers - 1 if tok else 0)


@pytest.mark.parametrize('tok', [False, True])
def test_generic_path_two_phases(dev, tok):
    """C1 (d_model 128): the generic GEMM path, with layer_tok the launches of layer_tok128"""
    from slotformer_amd import _lib, engine
    roll, _, _ = check_case(dev, 'c1', 2, 2, 12, 4, 404, {'layer_tok': tok})
    o = engine.rollout_opts({'layer_tok': tok})
    st = engine.rollouter_plan(roll).struct
    assert _lib.lib().sf_rollout_tok_layers(C.byref(st), 4, C.byref(o)) == (st.num_layers - 1 if tok else 0)


def test_fused_rows_without_ring(dev):
    """C4 (slot size 192: fused layers, no projection ring): the window staged, the out-projection's row map on groups of f frames"""
    check_case(dev, 'c4', 2, 2, 12, 3, 405)


@pytest.mark.parametrize('name', ['c2', 'c1'])
@torch.no_grad()
def test_stride_one_is_the_plain_rollout(dev, name):
    from slotformer_amd import engine
    roll, rd = rollouter(dev, name)
    hist, N, Cs = rd['history_len'], rd['num_slots'], rd['slot_size']
    x = gu.seeded_normal((3, hist + 5, N, Cs), 406).to(dev)
    a, b = x.clone(), x.clone()
    engine.rollout(roll, a, hist, 5)
    engine.rollout_phases(roll, b, hist, 5, 1)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    for opts in ({'seam': False}, {'layer_tok': True}):
        a, b = x.clone(), x.clone()
        engine.rollout(roll, a, hist, 4, opts=opts)
        engine.rollout_phases(roll, b, hist, 4, 1, opts=opts)
        torch.cuda.synchronize()
        assert torch.equal(a[:, :hist + 4], b[:, :hist + 4]) and torch.equal(b[:, hist + 4:], x[:, hist + 4:])
    # more observed frames than the burn-in: the window starts at frame obs - hist
    y = gu.seeded_normal((3, hist + 3 + 4, N, Cs), 407).to(dev)
    a, b = y[:, 3:].contiguous(), y.clone()
    engine.rollout(roll, a, hist, 4)
    engine.rollout_phases(roll, b, hist + 3, 4, 1)
    torch.cuda.synchronize()
    assert torch.equal(b[:, 3:], a) and torch.equal(b[:, :3], y[:, :3])


@torch.no_grad()
def test_stride_one_single_step_rollouter(dev):
    """the single-step rollouter (burn-in of one frame, a window growing to cond_len) takes frame_offset 1: the plain rollout's bits"""
    from slotformer_amd import engine
    from slotformer_amd.video_prediction.models import SingleStepSlotRollouter
    rd = gu.C5_ROLL['rollout_dict']
    torch.manual_seed(15)
    roll = SingleStepSlotRollouter(**rd).eval().to(dev)
    x = gu.seeded_normal((3, 2 + 8, rd['num_slots'], rd['slot_size']), 408).to(dev)
    a, b = x[:, 1:].contiguous(), x.clone()
    engine.rollout(roll, a, 1, 8)
    engine.rollout_phases(roll, b, 2, 8, 1)   # two observed frames: the burn-in is the last one
    torch.cuda.synchronize()
    assert torch.equal(b[:, 1:], a) and torch.equal(b[:, :2], x[:, :2])
    with pytest.raises(ValueError, match='frame_offset 1 only'):
        engine.rollout_phases(roll, b, 2, 8, 2)


@torch.no_grad()
def test_harness_one_call_on_the_h2_golden(dev):
    """the model and inputs of test_harness_gpu.test_h2_rollout_video_slots, held to that test's own bound"""
    from slotformer_amd.harness import rollout_video_slots
    g = gu.load_golden('harness_h2')
    m, _ = build(gu.C1_ROLL, g, 301, dev, vp=True)
    N, Cs = 6, 128
    ori = torch.stack([gu.seeded_normal((128, N, Cs), 301 + 10 + i) for i in range(2)])
    f = int(g['frame_offset'])
    out = rollout_video_slots(m, ori, f, one_call=True)
    assert out.shape == (2, 160, N, Cs)
    assert torch.equal(out[:, :128].cpu(), ori)
    e = rel_err(out, g['slots'])
    serial = rollout_video_slots(m, ori, f)
    d = ((out - serial).abs().max() / serial.abs().max()).item()
    print(f'harness_h2 golden, frame_offset {f}: one call rel err {e:.3e}; one call vs one call per phase {d:.3e}')
    assert e < 2e-4
    if exact(m.rollouter, None):
        assert torch.equal(out, serial)
    else:
        assert _close(out, serial)
    # an odd target length: the padded step is cut off
    out2 = rollout_video_slots(m, ori[:, :20], f, obs_frames=20, target_len=20 + 2 * f + 1, one_call=True)
    ser2 = rollout_video_slots(m, ori[:, :20], f, obs_frames=20, target_len=20 + 2 * f + 1)
    assert out2.shape == ser2.shape and _close(out2, ser2) and torch.equal(out2[:, :20].cpu(), ori[:, :20])


@torch.no_grad()
def test_captured_in_a_graph(dev):
    """the C2 case captured in one graph and replayed twice: the bits of the eager call both times"""
    from slotformer_amd import engine
    roll, buf, eager = check_case(dev, 'c2', 3, 2, 14, 5, 401)
    gbuf = buf.clone()
    engine.rollout_phases(roll, gbuf, 14, 5, 2)   # (warm: the workspace and the packed copies exist before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        engine.rollout_phases(roll, gbuf, 14, 5, 2)
    for _ in range(2):
        gbuf.copy_(buf)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gbuf, eager)
