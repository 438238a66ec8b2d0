"""CPU: the host side of video_prediction.fit -- the clip index (the reference dataset's rules), the schedule, the decaying step weights -- and the
argument checks of the clip entry points (csrc/clip_train.hip), which are raised before any HIP call."""
import ctypes as C
import json
import os

import pytest
import torch

import slotformer_fit_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- clip_index ---------------------------------------------------------------------------------------------------------------------------
def test_clip_index_by_hand():
    """video_len 12, 4 frames 2 apart: a clip spans frames s .. s + 6, so starts 0..5 fit; val cuts blocks of 8 frames and takes their 2
    interleaved clips."""
    from slotformer_amd.video_prediction import clip_index
    got = clip_index(2, 12, 4, 2, 'train')
    assert got.dtype == torch.int32 and got.tolist() == [[v, s] for v in range(2) for s in range(6)]
    assert clip_index(2, 12, 4, 2, 'val').tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert clip_index(1, 16, 4, 2, 'test').tolist() == [[0, 0], [0, 1], [0, 8], [0, 9]]
    assert clip_index(1, 5, 4, 2, 'train').shape == (0, 2)   # no clip fits


def test_clip_index_enter_times_by_hand():
    """warmup_len 4: a start s is dropped when an object enters at t with s + 2 < t <= s + 6.  Video 0 (t = 5): s = 3 has t == s + 2, the open
    end, and stays; s = 0..2 go.  Video 1 (t = 8): s = 2 has t == s + 6, the closed end, and goes, like s = 3..5; s = 0, 1 stay.  Video 2: nothing
    enters."""
    from slotformer_amd.video_prediction import clip_index
    enter = [[5], [8], []]
    train = clip_index(3, 12, 4, 2, 'train', enter_times=enter, warmup_len=4)
    assert train.tolist() == [[0, 3], [0, 4], [0, 5], [1, 0], [1, 1]] + [[2, s] for s in range(6)]
    # val: blocks of half a span (3 starts each: 0..2, 3..5), the first surviving start of each
    val = clip_index(3, 12, 4, 2, 'val', enter_times=enter, warmup_len=4)
    assert val.tolist() == [[0, 3], [1, 0], [2, 0], [2, 3]]
    # the default warm-up is the dataset's 5: the window opens at s + 4
    assert clip_index(1, 12, 4, 2, 'train', enter_times=[[4]]).tolist() == [[0, s] for s in range(6)]
    assert clip_index(1, 12, 4, 2, 'train', enter_times=[[5]]).tolist() == [[0, s] for s in range(1, 6)]
    with pytest.raises(ValueError):
        clip_index(2, 12, 4, 2, 'train', enter_times=[[1]])
    with pytest.raises(ValueError):
        clip_index(2, 12, 4, 2, 'training')


def test_clip_index_matches_recorded_reference():
    """tests/golden/clip_index_reference.json: the pairs the reference's CLEVRERDataset index methods (_get_sample_idx, _get_filtered_sample_idx)
    gave, driven without the dataset's I/O, for five shapes x three splits, with and without enter times."""
    from slotformer_amd.video_prediction import clip_index
    cases = json.load(open(os.path.join(GOLDEN, 'clip_index_reference.json')))
    assert len(cases) == 30
    for c in cases:
        want = c.pop('pairs')
        assert clip_index(**c).tolist() == want, c


# ---- clip_schedule ------------------------------------------------------------------------------------------------------------------------
def test_clip_schedule():
    from slotformer_amd.video_prediction import clip_schedule
    a, b = clip_schedule(10, 3, 4, 7), clip_schedule(10, 3, 4, 7)
    torch.manual_seed(123)   # (the global generator plays no part)
    c = clip_schedule(10, 3, 4, 7)
    for x, y, z in zip(a, b, c):
        assert len(x) == 2 and all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(x, y, z))
        assert all(t.dtype == torch.int32 and t.numel() == 4 for t in x)
    assert not all(torch.equal(p, q) for p, q in zip(a[0], a[1]))                 # the epochs continue one stream
    assert not all(torch.equal(p, q) for p, q in zip(a[0], clip_schedule(10, 3, 4, 8)[0]))
    full = clip_schedule(10, 2, 4, 7, drop_last=False)
    for e, kept in zip(full, a):
        assert [t.numel() for t in e] == [4, 4, 2]
        assert sorted(torch.cat(e).tolist()) == list(range(10))                   # every clip once per epoch
        assert all(torch.equal(p, q) for p, q in zip(e, kept))                    # drop_last drops the ragged batch, nothing else
    assert [len(e) for e in clip_schedule(8, 2, 4, 0)] == [2, 2]                   # nothing ragged: nothing dropped
    assert clip_schedule(3, 2, 4, 0) == [[], []]
    with pytest.raises(ValueError):
        clip_schedule(0, 1, 4, 0)


# ---- loss_decay_weights -------------------------------------------------------------------------------------------------------------------
def test_loss_decay_weights():
    from slotformer_amd.video_prediction import loss_decay_weights, loss_decay_factor
    total, pct, S = 200, 0.2, 10
    for step in (0, 1, 17, 39):
        f = 0.01 + step / (pct * total) * 0.99                                    # method.py:46-48
        assert loss_decay_factor(step, total, pct) == f
        w = torch.tensor(f, dtype=torch.float64)**torch.arange(S, dtype=torch.float64)   # slotformer.py:299-304
        w = w / w.sum() * S
        got = loss_decay_weights(step, total, pct, S)
        assert got.dtype == torch.float64 and torch.equal(got, w)
        assert abs(float(got.sum()) - S) < 1e-12
    for step in (40, 41, 199):                                                    # uniform from decay_pct * total on
        assert loss_decay_weights(step, total, pct, S) is None
    assert loss_decay_weights(0, total, None, S) is None
    assert loss_decay_weights(0, total, 0., S) is None


# ---- the C entry points reject bad arguments without a GPU --------------------------------------------------------------------------------
def _rollouter_struct():
    from slotformer_amd import _lib
    m = _lib.sf_rollouter(num_slots=3, slot_size=64, d_model=64, num_layers=2, num_heads=2, ffn_dim=64, norm_first=1, window_len=2, single_step=0)
    layers = (_lib.sf_tfm_layer * 2)()
    m.layers = C.cast(layers, C.POINTER(_lib.sf_tfm_layer))
    return m, layers


def test_clip_entry_points_reject_bad_arguments():
    from slotformer_amd import _lib
    lib = _lib.lib()

    def err():
        return lib.sf_last_error_string().decode()

    one = C.c_void_p(16)   # a non-null, 16-byte aligned dummy: every case below is rejected before it is dereferenced
    m, keep = _rollouter_struct()
    big = 1 << 40
    need = lib.sf_rollout_train_workspace_bytes(C.byref(m), 2, 3)
    assert need > 0
    fwd = lib.sf_rollout_train_clips_fwd_f32
    assert fwd(C.byref(m), None, 12, one, one, 2, one, 2, 3, 0., 0, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(C.byref(m), one, 12, None, one, 2, one, 2, 3, 0., 0, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(None, one, 12, one, one, 2, one, 2, 3, 0., 0, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(C.byref(m), one, 12, one, one, 0, one, 2, 3, 0., 0, one, big, None) < 0 and 'frame_offset' in err()
    assert fwd(C.byref(m), one, 12, one, one, 2, one, 0, 3, 0., 0, one, big, None) < 0 and 'B >= 1' in err()
    assert fwd(C.byref(m), one, 12, one, one, 2, one, 2, 3, 0., 0, one, need - 1, None) < 0 and 'workspace too small' in err()
    # 2 + 3 frames 2 apart span 9 frames: they fit 9, not 8
    assert fwd(C.byref(m), one, 8, one, one, 2, one, 2, 3, 0., 0, one, big, None) < 0 and 'does not fit' in err()
    assert fwd(C.byref(m), one, 12, one, one, 2, one, 2, 3, 1., 0, one, big, None) < 0 and 'dropout_p' in err()
    assert fwd(C.byref(m), C.c_void_p(20), 12, one, one, 2, one, 2, 3, 0., 0, one, big, None) < 0 and 'aligned' in err()

    mse = lib.sf_clip_mse_f32
    wsb = lib.sf_clip_mse_workspace_bytes(2, 3, 192)
    assert wsb > 0 and lib.sf_clip_mse_workspace_bytes(2, 65, 192) == 0 and lib.sf_clip_mse_workspace_bytes(2, 3, 190) == 0
    assert mse(None, one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 2, 3, 192, one, big, None) < 0 and 'null pointer' in err()
    assert mse(one, one, one, one, 12, 4, 2, None, None, 2, 1., one, None, 2, 3, 192, one, big, None) < 0 and 'null pointer' in err()
    assert mse(one, one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 0, 3, 192, one, big, None) < 0 and 'B >= 1' in err()
    assert mse(one, one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 2, 65, 192, one, big, None) < 0 and 'steps' in err()
    assert mse(one, one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 2, 3, 190, one, big, None) < 0 and 'multiple of 4' in err()
    assert mse(one, one, one, one, 12, 4, 0, None, None, 2, 1., one, one, 2, 3, 192, one, big, None) < 0 and 'frame_step' in err()
    # targets at frames 4, 6, 8 fit 9 frames, not 8
    assert mse(one, one, one, one, 8, 4, 2, None, None, 2, 1., one, one, 2, 3, 192, one, big, None) < 0 and 'do not fit' in err()
    assert mse(one, one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 2, 3, 192, one, wsb - 1, None) < 0 and 'workspace too small' in err()
    assert mse(C.c_void_p(20), one, one, one, 12, 4, 2, None, None, 2, 1., one, one, 2, 3, 192, one, big, None) < 0 and 'aligned' in err()

    frames = lib.sf_clip_frames_f32
    mean, std, zero = (C.c_float * 3)(.5, .5, .5), (C.c_float * 3)(.5, .5, .5), (C.c_float * 3)(.5, 0., .5)
    assert frames(None, 12, one, one, 4, 2, mean, std, one, 2, 3, 8, 8, None) < 0 and 'null pointer' in err()
    assert frames(one, 12, one, one, 4, 2, mean, std, one, 0, 3, 8, 8, None) < 0 and 'B >= 1' in err()
    assert frames(one, 12, one, one, 4, 0, mean, std, one, 2, 3, 8, 8, None) < 0 and 'frame_step' in err()
    assert frames(one, 8, one, one, 4, 2, mean, std, one, 2, 3, 8, 8, None) < 0 and 'do not fit' in err()
    assert frames(one, 12, one, one, 4, 2, mean, zero, one, 2, 3, 8, 8, None) < 0 and 'std' in err()
    assert frames(one, 12, one, one, 4, 2, mean, std, one, 2, 3, 0, 8, None) < 0 and 'frame size' in err()
    del keep


# ---- no CPU fallback ----------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise(tmp_path):
    from slotformer_amd import train, video_prediction as vp
    model = fc.build_model(fc.decoder_checkpoint(str(tmp_path / 'dec.pth')))
    table = fc.seeded_table()
    clips = vp.clip_index(fc.V, fc.T, fc.HIST + fc.S, 2, 'train')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vp.fit(model, table, clips, 1, 2, 1e-3, 0, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vp.evaluate(model, table, clips, 2, 2)
    cv, cs = clips[:2, 0].contiguous(), clips[:2, 1].contiguous()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.rollout_clips_with_grad(model.rollouter, table, cv, cs, 2, fc.S)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.clip_mse(torch.zeros(2, 3, 8), torch.zeros(2, 3, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.clip_frames(torch.zeros(2, 12, 8, 8, 3, dtype=torch.uint8), cv, cs, 2, fc.HIST, fc.S)


def test_stack_slot_table():
    import numpy as np
    from slotformer_amd import slot_io
    d = {'b.mp4': np.ones((4, 3, 8), np.float64), 'a.mp4': np.zeros((4, 3, 8), np.float32)}
    table, names = slot_io.stack_slot_table(d)
    assert names == ['a.mp4', 'b.mp4'] and table.dtype == np.float32 and table.shape == (2, 4, 3, 8) and table[1].min() == 1
    table, names = slot_io.stack_slot_table(d, names=['/videos/b.mp4'])
    assert names == ['b.mp4'] and table.shape == (1, 4, 3, 8)
    d['c.mp4'] = np.zeros((5, 3, 8), np.float32)
    with pytest.raises(ValueError):
        slot_io.stack_slot_table(d)
