"""CPU: the rollout at a frame offset (sf_rollout_phases_f32 / engine.rollout_phases) -- its workspace, its argument errors (all raised
before any HIP call, so they are testable without a GPU) and the frame table a phase reads and writes, stated in plain Python and held
against the reference driver's gather (`full[:, start::f]`) and interleave (rollout_clevrer_slots.py:20-65)."""
import ctypes as C

import pytest
import torch

from slotformer_amd import configs
from test_rollout_plan import rollouter, SHAPES

ONE = 16   # a non-null dummy pointer: every case below is refused before it is dereferenced


@pytest.fixture
def lib():
    from slotformer_amd import _lib
    return _lib.lib()


def err(lib):
    return lib.sf_last_error_string().decode()


def test_workspace_is_that_of_the_virtual_videos(lib):
    assert lib.sf_rollout_phases_workspace_bytes(None, 4, 2) == 0
    for name, (cfg, window) in SHAPES.items():
        m = rollouter(cfg, window)
        for B, f in ((1, 1), (1, 2), (3, 2), (32, 3), (5, 3)):
            assert lib.sf_rollout_phases_workspace_bytes(C.byref(m), B, f) == lib.sf_rollout_workspace_bytes(C.byref(m), B * f) > 0, (name, B, f)
        assert lib.sf_rollout_phases_workspace_bytes(C.byref(m), 0, 2) == 0
        assert lib.sf_rollout_phases_workspace_bytes(C.byref(m), 2, 0) == 0


def call(lib, m, B, T_total, obs, f, pred_len, slots=ONE, ws=ONE, ws_bytes=1 << 40):
    return lib.sf_rollout_phases_f32(C.byref(m) if m is not None else None, C.cast(slots, C.POINTER(C.c_float)) if slots else None, B, T_total, obs,
                                     f, pred_len, ws, ws_bytes, None, None)


def test_c_entry_refuses_bad_arguments_before_any_launch(lib):
    m = rollouter(configs.C2_ROLL)   # hist 6
    assert call(lib, m, 3, 21, 14, 0, 5) < 0 and 'frame_offset >= 1' in err(lib)
    assert call(lib, m, 3, 21, 14, -1, 5) < 0 and 'frame_offset >= 1' in err(lib)
    assert call(lib, m, 3, 21, 11, 2, 5) < 0 and 'fewer observed frames' in err(lib)        # obs < hist * f
    assert call(lib, m, 3, 19, 14, 2, 5) < 0 and 'slots buffer shorter' in err(lib)         # S = 3: 20 frames are written, T_total one short
    assert call(lib, m, 3, 17, 14, 2, 4) < 0 and 'slots buffer shorter' in err(lib)         # S = 2: 18 frames
    assert call(lib, m, 0, 21, 14, 2, 5) < 0 and 'bad batch' in err(lib)
    assert call(lib, m, 3, 21, 14, 2, -1) < 0 and 'bad batch' in err(lib)
    for kw in (dict(slots=None), dict(ws=None)):
        assert call(lib, m, 3, 21, 14, 2, 5, **kw) < 0 and 'null pointer' in err(lib)
    assert call(lib, None, 3, 21, 14, 2, 5) < 0 and 'null pointer' in err(lib)
    assert call(lib, m, 3, 21, 14, 2, 5, ws_bytes=lib.sf_rollout_workspace_bytes(C.byref(m), 6) - 1) < 0 and 'workspace too small' in err(lib)
    assert call(lib, m, 3, 21, 14, 2, 5, ws_bytes=lib.sf_rollout_workspace_bytes(C.byref(m), 3)) < 0 and 'workspace too small' in err(lib)
    single = rollouter(configs.C5_ROLL)
    assert call(lib, single, 2, 40, 12, 2, 4) < 0 and 'single-step' in err(lib)
    from slotformer_amd import _lib
    o = _lib.sf_rollout_opts(-1, -1, 48, 0, 0, 0, 0, 0)   # ffn_rows 48: the options are checked as sf_rollout_opts_f32 checks them
    rc = lib.sf_rollout_phases_f32(C.byref(m), C.cast(ONE, C.POINTER(C.c_float)), 3, 21, 14, 2, 5, ONE, 1 << 40, None, C.byref(o))
    assert rc < 0 and 'ffn_rows' in err(lib)


def _modules():
    from slotformer_amd.video_prediction.models import SlotRollouter, SingleStepSlotRollouter
    roll = SlotRollouter(**configs.C2_ROLL['rollout_dict']).eval()
    single = SingleStepSlotRollouter(**configs.C5_ROLL['rollout_dict']).eval()
    return roll, single


@torch.no_grad()
def test_engine_entry_refuses_bad_arguments_before_the_c_call():
    from slotformer_amd import engine
    roll, single = _modules()
    buf = torch.zeros(3, 21, 7, 128)
    with pytest.raises(ValueError, match='frame_offset >= 1'):
        engine.rollout_phases(roll, buf, 14, 5, 0)
    with pytest.raises(ValueError, match='observed frames'):
        engine.rollout_phases(roll, buf, 11, 5, 2)
    with pytest.raises(ValueError, match='pad it'):
        engine.rollout_phases(roll, buf[:, :19].contiguous(), 14, 5, 2)   # S = 3: 20 frames are written
    with pytest.raises(ValueError, match='frame_offset 1 only'):
        engine.rollout_phases(single, torch.zeros(2, 40, 8, 128), 12, 4, 2)
    with pytest.raises(ValueError, match=r'\[B, T_total, N, C\]'):
        engine.rollout_phases(roll, buf[0], 14, 5, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.rollout_phases(roll, buf, 14, 5, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.rollout_phases(roll, buf[:, :20].contiguous(), 14, 5, 2)   # exactly obs + S * f frames: accepted up to the device check


@torch.no_grad()
def test_harness_one_call_keyword():
    """one_call defaults to False (the reference's restatement); True goes to engine.rollout_phases, which has no CPU fallback, and takes the
    rollouter's own burn-in only."""
    import inspect
    from slotformer_amd import harness
    assert inspect.signature(harness.rollout_video_slots).parameters['one_call'].default is False

    class Model:
        history_len = 6
        device = torch.device('cpu')
        rollouter = _modules()[0]

        def eval(self):
            return self

    ori = torch.zeros(1, 14, 7, 128)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harness.rollout_video_slots(Model(), ori, 2, obs_frames=14, target_len=19, one_call=True)
    with pytest.raises(ValueError, match='burn-in'):
        harness.rollout_video_slots(Model(), ori, 2, history_len=5, obs_frames=14, target_len=19, one_call=True)


# ---- the frame table -----------------------------------------------------------------------------------------------------------------
def phase_frames(obs, hist, f, pred_len):
    """What sf_rollout_phases_f32 promises: per phase p, the frames it burns in on and the frame each of its S steps writes."""
    first, S = obs - hist * f, -(-pred_len // f)
    return [([first + p + j * f for j in range(hist)], [obs + p + s * f for s in range(S)]) for p in range(f)]


@pytest.mark.parametrize('obs,hist,f,pred_len', [(14, 6, 2, 5), (45, 15, 3, 7), (128, 6, 2, 32), (6, 6, 1, 4)])
def test_frame_table_is_the_reference_gather_and_interleave(obs, hist, f, pred_len):
    target_len = obs + pred_len
    S = -(-pred_len // f)
    table = phase_frames(obs, hist, f, pred_len)
    full = torch.arange(target_len).reshape(1, target_len)   # a "video" whose frame t holds t
    written = {}
    for off in range(f):
        start = obs - hist * f + off                           # rollout_clevrer_slots.py:40-47
        idx = full[:, start::f][0].tolist()
        rollout_len = len(idx) - hist
        burn, wr = table[off]
        assert idx[:hist] == burn
        assert idx[hist:] == wr[:rollout_len]                  # the frames the reference's phase predicts are this phase's first steps ...
        assert S - rollout_len in (0, 1) and all(t >= target_len for t in wr[rollout_len:])   # ... at most one more, in the padding
        for s, t in enumerate(wr):
            assert t not in written
            written[t] = (off, s)
    # every frame of [obs, obs + S f) is written exactly once, nothing before obs; frames before `first` belong to no phase
    assert sorted(written) == list(range(obs, obs + S * f))
    assert min(min(b) for b, _ in table) == obs - hist * f and max(max(b) for b, _ in table) == obs - 1
    # the reference's interleave (rollout_clevrer_slots.py:56-59): predicted frame i comes from phase i % f, step i // f
    for i in range(pred_len):
        assert written[obs + i] == (i % f, i // f)
    # virtual video v = b f + p of the flattened buffer: base b * bs + (first + p) * NC, frame stride f * NC -- frame u of v is
    # frame first + p + u f of video b (the burn-in u < hist, step s writes u = hist + s)
    first = obs - hist * f
    for p, (burn, wr) in enumerate(table):
        assert [first + p + u * f for u in range(hist + S)] == burn + wr
