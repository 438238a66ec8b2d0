"""CPU: what `base_slots.fit` rests on that needs no device -- the host twin of the in-kernel normal noise (its statistics at 5-sigma sampling
bounds), the schedules by hand, the refusals of `fit` before any device work, and the argument errors of the three C entry points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import base_fit_cases as bc

N = 1 << 20
SEEDS = (1, 0x0badc0de12345678, 2**62 - 5)
TAGS = (0, 1, 5)


@pytest.fixture(scope='module')
def noise():
    """train.normal_noise at n = 2^20 for every (seed, tag) pair and for tag + 1, float64 copies, computed once"""
    from slotformer_amd import train
    return {(s, t): train.normal_noise(s, t, N).numpy().astype(np.float64) for s in SEEDS for t in sorted(set(TAGS) | {t + 1 for t in TAGS})}


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('seed', SEEDS)
def test_normal_noise_statistics(noise, seed, tag):
    """5-sigma sampling bounds of n = 2^20 independent standard normals (the variance of each estimator under the null; not measurements):
    mean, lag-1 autocorrelation, correlation with the next tag: 5 / sqrt(n); variance: 5 sqrt(2 / n); fourth moment: 5 sqrt(96 / n);
    P(|eps| > 3) = 0.0027: 5 sqrt(p / n) = 0.00026; |eps| <= sqrt(-2 ln 2^-24) = 5.77."""
    e = noise[(seed, tag)]
    got = {'mean': abs(e.mean()), 'var': abs(e.var() - 1.), 'autocorr': abs(_corr(e[:-1], e[1:])), 'crosscorr': abs(_corr(e, noise[(seed, tag + 1)])),
           'fourth': abs((e**4).mean() - 3.), 'tail': abs((np.abs(e) > 3.).mean() - 0.0027), 'max': np.abs(e).max()}
    print(seed, tag, {k: round(float(v), 5) for k, v in got.items()})
    assert got['mean'] < 5 / math.sqrt(N)
    assert got['autocorr'] < 5 / math.sqrt(N)
    assert got['crosscorr'] < 5 / math.sqrt(N)
    assert got['var'] < 5 * math.sqrt(2 / N)
    assert got['fourth'] < 5 * math.sqrt(96 / N)
    assert got['tail'] < 0.00026
    assert got['max'] <= 5.78


def test_normal_noise_is_a_function_of_its_arguments():
    from slotformer_amd import train
    a = train.normal_noise(SEEDS[1], 3, 4096)
    assert a.dtype == torch.float32 and tuple(a.shape) == (4096, )
    assert torch.equal(a, train.normal_noise(SEEDS[1], 3, 4096))
    assert torch.equal(a[:100], train.normal_noise(SEEDS[1], 3, 100))          # element i does not depend on the length
    assert not torch.equal(a, train.normal_noise(SEEDS[1], 4, 4096))
    assert not torch.equal(a, train.normal_noise(SEEDS[1] + 1, 3, 4096))
    assert not torch.equal(a, train.normal_noise(SEEDS[1] ^ (1 << 40), 3, 4096))   # the high half of the seed counts


# ---- schedules by hand ------------------------------------------------------------------------------------------------------------------------
def test_cosine_anneal_by_hand():
    from slotformer_amd.base_slots import cosine_anneal
    assert cosine_anneal(0, 1., 0.1, 30) == pytest.approx(1.)
    assert cosine_anneal(15, 1., 0.1, 30) == pytest.approx(0.55)          # half-way: the mean of the two
    assert cosine_anneal(10, 1., 0.1, 30) == pytest.approx(0.45 * 0.5 + 0.55)   # cos(pi / 3) = 1 / 2
    assert cosine_anneal(30, 1., 0.1, 30) == 0.1
    assert cosine_anneal(31, 1., 0.1, 30) == 0.1 and cosine_anneal(10**6, 1., 0.1, 30) == 0.1
    assert cosine_anneal(3, 1., 0.1, 30, start_step=5) == 1.
    assert cosine_anneal(0, 1., 0.1, 0) == 0.1                            # nothing to anneal over


def test_steve_rates_by_hand():
    """STEVE's two groups: each its own warm-up and cosine to 0 (what fit assigns to FlatAdam.param_groups before every step)."""
    from slotformer_amd import train
    total, warm = 40, 0.05 * 40
    for peak in (1e-4, 3e-4):
        assert train.warmup_cosine_lr(0, total, warm, peak) == 0.
        assert train.warmup_cosine_lr(1, total, warm, peak) == pytest.approx(peak / 2)
        assert train.warmup_cosine_lr(2, total, warm, peak) == pytest.approx(peak)
        assert train.warmup_cosine_lr(21, total, warm, peak) == pytest.approx(peak / 2)      # half of the 38 cosine steps
        assert train.warmup_cosine_lr(40, total, warm, peak) == pytest.approx(0., abs=1e-12)
    m = bc.steve()
    groups = train.steve_param_groups(m, 1e-4, 3e-4)
    assert [g['lr'] for g in groups] == [1e-4, 3e-4]
    names = {id(p): n for n, p in m.named_parameters()}
    assert all('trans_decoder' in names[id(p)] for p in groups[1]['params']) and groups[1]['params']
    assert not any('trans_decoder' in names[id(p)] or names[id(p)].startswith('dvae.') for p in groups[0]['params'])


def test_clip_rules_are_reexported():
    from slotformer_amd import base_slots, video_prediction as vp
    assert base_slots.clip_index is vp.clip_index and base_slots.clip_schedule is vp.clip_schedule
    from slotformer_amd.base_slots import clip_index
    assert tuple(clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train').shape) == (bc.V * (bc.T - 1), 2)


# ---- fit refuses before any device work -----------------------------------------------------------------------------------------------------------
def test_fit_refusals_on_cpu_tensors():
    from slotformer_amd import base_slots as bs
    frames = bc.random_frames()
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')
    dv, sv, st = bc.dvae(), bc.savi(), bc.steve()
    args = (1, bc.BATCH, 1e-3, bc.SEED, bc.N_FRAMES)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bs.fit(dv, frames, clips, *args)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bs.evaluate(dv, frames, clips, bc.BATCH, bc.N_FRAMES)
    with pytest.raises(ValueError, match='contiguous uint8'):
        bs.fit(dv, frames.float(), clips, *args)
    with pytest.raises(ValueError, match='contiguous uint8'):
        bs.fit(dv, frames[:, :, :, :, :2], clips, *args)
    with pytest.raises(ValueError, match="at the model's resolution"):
        bs.fit(sv, frames[:, :, :32, :32].contiguous(), clips, *args)
    with pytest.raises(ValueError, match="at the model's resolution"):
        bs.evaluate(st, frames[:, :, :32].contiguous(), clips, bc.BATCH, bc.N_FRAMES)
    with pytest.raises(ValueError, match='multiples of 4'):
        bs.fit(dv, frames[:, :, :62].contiguous(), clips, *args)
    late = torch.tensor([[0, 0], [1, bc.T - 1]], dtype=torch.int32)    # 2 frames from T - 1: the last one is frame T
    with pytest.raises(ValueError, match='does not fit'):
        bs.fit(sv, frames, late, *args)
    with pytest.raises(ValueError, match='does not fit'):
        bs.evaluate(sv, frames, late, bc.BATCH, bc.N_FRAMES)
    assert bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')[:, 1].max() == bc.T - 2
    with pytest.raises(ValueError, match='tokens are contiguous int16 or int64'):
        bs.fit(st, frames, clips, *args, dec_lr=3e-4, tokens=torch.zeros(bc.V, bc.T, 255, dtype=torch.int64))
    with pytest.raises(ValueError, match='tokens are contiguous int16 or int64'):
        bs.fit(st, frames, clips, *args, dec_lr=3e-4, tokens=torch.zeros(bc.V, bc.T, 256, dtype=torch.int32))
    with pytest.raises(ValueError, match='tokens= are the targets'):
        bs.fit(sv, frames, clips, *args, tokens=torch.zeros(bc.V, bc.T, 256, dtype=torch.int64))
    with pytest.raises(ValueError, match='dec_lr'):
        bs.fit(st, frames, clips, *args)
    with pytest.raises(ValueError, match='do not fill one batch'):
        bs.fit(dv, frames, clips, 1, clips.shape[0] + 1, 1e-3, bc.SEED, bc.N_FRAMES)
    with pytest.raises(ValueError, match='n_sample_frames'):
        bs.fit(dv, frames, clips, 1, bc.BATCH, 1e-3, bc.SEED, 0)
    with pytest.raises(ValueError, match='loss_w'):
        bs.fit(sv, frames, clips, *args, loss_w=(1., ))


def test_node_and_ops_refuse_cpu_tensors():
    from slotformer_amd import ops, train
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.kernel_sample(torch.zeros(3, 16), 8, 0., seed=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.normal_noise(1, 0, 8, device='cpu')
    with pytest.raises(ValueError, match='noise= or seed='):
        train.kernel_sample(torch.zeros(3, 16), 8, 0.)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments():
    from slotformer_amd import _lib
    lib = _lib.lib()

    def err():
        return lib.sf_last_error_string().decode()

    one = C.c_void_p(16)   # a non-null, 16-byte aligned dummy: every case below is rejected before it is dereferenced
    big = 1 << 40
    assert lib.sf_normal_noise_f32(None, 8, 1, 0, None) < 0 and 'null pointer' in err()
    assert lib.sf_normal_noise_f32(one, 0, 1, 0, None) < 0 and '2^31 elements' in err()
    assert lib.sf_normal_noise_f32(one, (1 << 31) + 1, 1, 0, None) < 0 and '2^31 elements' in err()

    need = lib.sf_kernel_sample_workspace_bytes(300, 192)
    assert need == 16 + 8 * 57            # 14400 float4s in workgroups of 256: 57 partials behind the counter
    assert lib.sf_kernel_sample_workspace_bytes(1, 4) == 24 and lib.sf_kernel_sample_workspace_bytes(1 << 20, 1024) == 16 + 8 * 256
    assert lib.sf_kernel_sample_workspace_bytes(0, 64) == 0 and lib.sf_kernel_sample_workspace_bytes(3, 6) == 0
    assert lib.sf_kernel_sample_workspace_bytes(3, 1028) == 0 and lib.sf_kernel_sample_workspace_bytes((1 << 21) + 1, 1024) == 0
    fwd = lib.sf_kernel_sample_fwd_f32
    assert fwd(None, None, 1, 0, 0., one, one, 300, 192, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(one, None, 1, 0, 0., None, one, 300, 192, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(one, None, 1, 0, 0., one, None, 300, 192, one, big, None) < 0 and 'null pointer' in err()
    assert fwd(one, None, 1, 0, 0., one, one, 300, 192, None, big, None) < 0 and 'null pointer' in err()
    assert fwd(one, None, 1, 0, 0., one, one, 300, 6, one, big, None) < 0 and 'multiple of 4' in err()
    assert fwd(one, None, 1, 0, 0., one, one, 300, 1028, one, big, None) < 0 and 'at most 1024' in err()
    assert fwd(one, None, 1, 0, 0., one, one, 0, 192, one, big, None) < 0 and 'R >= 1' in err()
    assert fwd(one, None, 1, 0, 0., one, one, 300, 192, one, need - 1, None) < 0 and 'workspace too small' in err()
    assert fwd(one, C.c_void_p(20), 1, 0, 0., one, one, 300, 192, one, big, None) < 0 and 'aligned' in err()
    bwd = lib.sf_kernel_sample_bwd_f32
    assert bwd(None, None, 1, 0, 0., one, one, 1., one, 300, 192, None) < 0 and 'null pointer' in err()
    assert bwd(one, None, 1, 0, 0., one, None, 1., one, 300, 192, None) < 0 and 'null pointer' in err()
    assert bwd(one, None, 1, 0, 0., one, one, 1., None, 300, 192, None) < 0 and 'null pointer' in err()
    assert bwd(one, None, 1, 0, 0., one, one, 1., one, 300, 6, None) < 0 and 'multiple of 4' in err()
    assert bwd(one, None, 1, 0, 0., one, one, 1., one, 0, 192, None) < 0 and 'R >= 1' in err()
    assert bwd(one, None, 1, 0, 0., C.c_void_p(24), one, 1., one, 300, 192, None) < 0 and 'aligned' in err()
