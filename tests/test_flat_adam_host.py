"""CPU: the host side of FlatAdam's parameter groups -- the warm-up + cosine schedule, STEVE's two groups and the layout of the
groups in the flat bucket."""
import math

import pytest
import torch

import golden_util as gu


def _closed(step, total, warm, hi, lo):
    if step < warm:
        return lo + (hi - lo) * step / warm
    return lo + (hi - lo) * (1. + math.cos(math.pi * (step - warm) / (total - warm))) / 2.


# (max_lr, min_lr, warm-up share): the slot models (lr / 100, 2.5 %) and STEVE's two rates (0, 5 %)
@pytest.mark.parametrize('hi,lo,pct', [(2e-4, 2e-6, 0.025), (1e-4, 1e-6, 0.025), (1e-4, 0., 0.05), (3e-4, 0., 0.05)])
def test_warmup_cosine_lr(hi, lo, pct):
    from slotformer_amd.train import warmup_cosine_lr
    total = 4000
    warm = int(pct * total)
    mid = warm + (total - warm) // 2
    for step in (0, 1, warm - 1, warm, warm + 1, mid, total - 1, total):
        assert warmup_cosine_lr(step, total, warm, hi, lo) == pytest.approx(_closed(step, total, warm, hi, lo), rel=1e-12, abs=1e-20), step
    assert warmup_cosine_lr(0, total, warm, hi, lo) == lo
    assert warmup_cosine_lr(warm, total, warm, hi, lo) == hi
    assert warmup_cosine_lr(mid, total, warm, hi, lo) == pytest.approx((hi + lo) / 2, rel=1e-3)
    assert warmup_cosine_lr(total, total, warm, hi, lo) == pytest.approx(lo, abs=1e-18)
    seq = [warmup_cosine_lr(s, total, warm, hi, lo) for s in range(total + 1)]
    assert all(b > a for a, b in zip(seq[:warm], seq[1:warm + 1]))        # monotone up ...
    assert all(b < a for a, b in zip(seq[warm:-1], seq[warm + 1:]))       # ... then monotone down
    assert max(seq) == hi and min(seq) >= lo - 1e-18
    # no warm-up: the peak at step 0; a fractional warm-up length (a share of the steps) is taken as it is
    assert warmup_cosine_lr(0, total, 0, hi, lo) == hi
    assert warmup_cosine_lr(3, total, 7.5, hi, lo) == pytest.approx(lo + (hi - lo) * 3 / 7.5, rel=1e-12)


def test_steve_param_groups():
    from slotformer_amd.base_slots import build_model
    from slotformer_amd.train import steve_param_groups, flat_bucket_layout
    m = build_model(gu.ParamsView(gu.steve_tokens_cfg()))
    groups = steve_param_groups(m, 1e-4, 3e-4)
    assert [g['lr'] for g in groups] == [1e-4, 3e-4]
    named = dict(m.named_parameters())
    ids = [[id(p) for p in g['params']] for g in groups]
    dec = [n for n, p in named.items() if 'trans_decoder' in n and p.requires_grad]   # (its attention masks are fixed parameters)
    assert dec and all(id(named[n]) in ids[1] for n in dec) and len(ids[1]) == len(dec)
    assert not any(id(named[n]) in ids[0] for n in dec)
    frozen = [n for n, p in named.items() if not p.requires_grad]
    assert any(n.startswith('dvae.') for n in frozen)                      # the dVAE is frozen ...
    assert not any(id(named[n]) in ids[0] + ids[1] for n in frozen)       # ... and in neither group
    want = sorted(id(p) for p in named.values() if p.requires_grad)
    assert sorted(ids[0] + ids[1]) == want                                # every trainable parameter, each once
    params, begins = flat_bucket_layout(groups)
    assert begins == [0, sum(p.numel() for p in groups[0]['params'])]
    assert [id(p) for p in params] == ids[0] + ids[1]


def test_flat_bucket_layout():
    from slotformer_amd.train import flat_bucket_layout
    sizes = ((1, 7, 33), (255, ), (), (257, 1000))
    groups = [{'params': [torch.nn.Parameter(torch.zeros(k)) for k in ks], 'lr': 1e-3 * (i + 1)} for i, ks in enumerate(sizes)]
    groups[0]['params'].insert(1, torch.nn.Parameter(torch.zeros(5), requires_grad=False))   # frozen: takes no room
    params, begins = flat_bucket_layout(groups)
    run, want = 0, []
    for ks in sizes:
        want.append(run)
        run += sum(ks)
    assert begins == want == [0, 41, 296, 296]
    assert all(b >= a for a, b in zip(begins, begins[1:])) and begins[0] == 0
    assert [p.numel() for p in params] == [k for ks in sizes for k in ks]
    # a plain list of tensors is one group: FlatAdam's historical form
    assert flat_bucket_layout([{'params': params}])[1] == [0]


def test_flat_adam_needs_a_device():
    """The new keywords exist and the constructor still refuses CPU parameters: there is no fallback."""
    from slotformer_amd.train import FlatAdam
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(RuntimeError, match='HIP device'):
        FlatAdam([{'params': ps, 'lr': 1e-3}], lr=2e-4, clip_grad=0.05)
    with pytest.raises(ValueError, match='1 to 8'):
        FlatAdam([{'params': ps} for _ in range(9)])


def test_new_entry_points_reject_bad_arguments():
    """Argument errors come before any HIP call, so they are checked without a GPU too."""
    import ctypes as C
    from slotformer_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)
    g = (_lib.sf_adam_group * 2)()
    g[0].begin, g[1].begin = 0, 5
    assert lib.sf_adam_flat_groups_f32(one, one, one, one, 10, 1, g, 0, 0.9, 0.999, 1e-8, None, None) < 0
    assert 'groups' in lib.sf_last_error_string().decode()
    g[0].begin = 1
    assert lib.sf_adam_flat_groups_f32(one, one, one, one, 10, 1, g, 2, 0.9, 0.999, 1e-8, None, None) < 0
    assert 'begins at 0' in lib.sf_last_error_string().decode()
    assert lib.sf_grad_clip_coef_f32(one, 10, 0.05, one, one, lib.sf_grad_norm_workspace_bytes(10) - 1, None) < 0
    assert 'workspace' in lib.sf_last_error_string().decode()
    assert lib.sf_grad_norm_workspace_bytes(10) == 32 and lib.sf_grad_norm_workspace_bytes(1 << 40) == 16 + 16 * 1024
