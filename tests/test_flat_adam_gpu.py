"""GPU: gradient clipping and parameter groups of train.FlatAdam -- sf_grad_clip_coef_f32 (global norm, clip coefficient,
non-finite flag in one launch) and sf_adam_flat_groups_f32 (Adam with per-group rates and a device-side gradient scale)
against float64, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam with param groups."""
import pytest
import torch

import golden_util as gu
from test_engine_gpu import rel_err

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 33, 255, 257, 1000, 3, 129, 511, 64, 2049)   # eleven tensors of odd sizes, split 6 / 5


def _lib():
    from slotformer_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(n, dev):
    return torch.zeros(int(_lib().lib().sf_grad_norm_workspace_bytes(n)), dtype=torch.uint8, device=dev)


def _clip(g, max_norm, ws, out=None):
    out = torch.zeros(3, dtype=torch.float32, device=g.device) if out is None else out
    _lib().check(_lib().lib().sf_grad_clip_coef_f32(g.data_ptr(), g.numel(), float(max_norm), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _stream()))
    return out


def _bar(g, own=None):
    """The bar of the norm: twice the relative distance of torch's own fp32 norm (`own`; default torch.linalg.vector_norm of the
    bucket) from the float64 value, and never more than 1e-6 -- fp32 accumulation runs over a thread's own few elements only,
    everything after is double, so the kernel is about as close to float64 as a float can be.  Returns (float64 norm, bar)."""
    ref = torch.linalg.vector_norm(g.double()).item()
    own = torch.linalg.vector_norm(g).item() if own is None else own
    d = abs(own - ref) / ref if ref > 0 else 0.
    return ref, min(2 * d, 1e-6)


def _grid(n):
    from slotformer_amd import train
    return train.grad_norm_grid(n)


def _norm_sizes():
    big = _grid(1 << 40)   # the full grid
    return (1, 3, 255, 256, 257, 1023, 1025, big * 256 * 4 + 1, 1000003)


@pytest.fixture(scope='module')
def normal_pool(dev):
    """Seeded normal gradients * 0.1, one float longer than the largest bucket (for the runs from an odd base pointer)."""
    n = max(_norm_sizes()) + 1
    g = torch.Generator(device='cpu').manual_seed(11)
    return (torch.randn(n, generator=g) * 0.1).to(dev)


@pytest.mark.parametrize('offset', [0, 1])
def test_norm_against_float64(dev, normal_pool, offset):
    assert _grid(_norm_sizes()[-2]) == _grid(1 << 40) and _norm_sizes()[-2] > _grid(1 << 40) * 256 * 4   # some thread strides on
    for n in _norm_sizes():
        g = normal_pool[offset:offset + n]
        assert g.data_ptr() % 16 == 4 * offset
        ws = _ws(n, dev)
        out = _clip(g, 0.05, ws)
        ref, bar = _bar(g)
        got = out[0].item()
        err = abs(got - ref) / ref
        print(f'n={n} offset={offset} norm={got:.9g} f64={ref:.12g} rel={err:.3g} bar={bar:.3g}')
        assert err <= bar, (n, err, bar)
        assert out[2].item() == 0.
        again = _clip(g, 0.05, ws)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32)), n   # identical bits from call to call
        assert ws[:4].view(torch.int32).item() == 0   # the arrival counter is back at zero


def test_norm_workspace_reuse(dev, normal_pool):
    """One workspace, zeroed once, serves calls with different n (different grids) one after the other."""
    ws = _ws(1000003, dev)
    for n in (1000003, 257, 70001, 1, 1000003):
        g = normal_pool[:n]
        out = _clip(g, 0.05, ws)
        ref, bar = _bar(g)
        assert abs(out[0].item() - ref) / ref <= bar, n
        assert ws[:4].view(torch.int32).item() == 0


def test_coefficient_rule(dev):
    gen = torch.Generator(device='cpu').manual_seed(5)
    base = torch.randn(5001, generator=gen).to(dev)
    ws = _ws(base.numel(), dev)
    # norm above max_norm: torch's coefficient; below: exactly 1; all-zero: exactly 1
    for scale, clipped in ((0.1, True), (1e-5, False), (0., False)):
        g = base * scale
        p = torch.nn.Parameter(torch.zeros_like(g))
        p.grad = g.clone()
        tnorm = torch.nn.utils.clip_grad_norm_([p], 0.05).item()
        out = _clip(g, 0.05, ws).cpu()
        ref, bar = _bar(g, tnorm)
        print(f'scale={scale} norm={out[0].item():.9g} torch={tnorm:.9g} f64={ref:.12g} bar={bar:.3g} coef={out[1].item():.9g}')
        assert (tnorm > 0.05) == clipped
        if ref > 0:
            assert abs(out[0].item() - ref) / ref <= bar
        else:
            assert out[0].item() == 0. and tnorm == 0.
        if clipped:
            # the rule itself, exactly: max_norm / (norm + 1e-6) in fp32 on the norm that was written ...
            assert out[1].item() == (torch.tensor(0.05) / (out[0] + 1e-6)).item()
            # ... so the coefficient is as far from the float64 one (of the fp32 max_norm) as the norm is (the bar) plus the
            # roundings of one fp32 sum and one fp32 quotient, and it is what clip_grad_norm_ multiplied the gradient by
            want = torch.tensor(0.05).item() / (ref + 1e-6)
            assert abs(out[1].item() - want) / want <= bar + 2 * 2.0**-24
            assert rel_err(g * out[1].item(), p.grad.cpu()) <= 1e-6
        else:
            assert out[1].item() == 1.0
            assert torch.equal(p.grad, g)
        assert out[2].item() == 0.
    # max_norm <= 0: no clipping
    assert _clip(base, 0., ws)[1].item() == 1.0
    # one NaN / one Inf at the last element raise the flag
    for badv in (float('nan'), float('inf'), float('-inf')):
        for n in (5001, 1, 1027):
            g = (base[:n] * 0.1).clone()
            g[-1] = badv
            out = _clip(g, 0.05, ws)
            assert out[2].item() == 1.0, (badv, n)
    assert _clip(base * 0.1, 0.05, ws)[2].item() == 0.


def _groups(pairs):
    arr = (_lib().sf_adam_group * len(pairs))()
    for a, (b, lr) in zip(arr, pairs):
        a.begin, a.lr = b, lr
    return arr


def test_one_group_equals_plain_kernel(dev):
    n = 70001
    gen = torch.Generator(device='cpu').manual_seed(21)
    p0 = torch.randn(n, generator=gen).to(dev)
    state = [[p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)] for _ in range(2)]
    lib = _lib().lib()
    for step in range(1, 6):
        g = (torch.randn(n, generator=gen) * 0.1).to(dev)
        (pa, ma, va), (pb, mb, vb) = state
        _lib().check(lib.sf_adam_flat_f32(pa.data_ptr(), g.data_ptr(), ma.data_ptr(), va.data_ptr(), n, step, 2e-4, 0.9, 0.999, 1e-8, _stream()))
        _lib().check(lib.sf_adam_flat_groups_f32(pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), n, step, _groups([(0, 2e-4)]), 1,
                                                 0.9, 0.999, 1e-8, None, _stream()))
    for a, b, name in zip(state[0], state[1], ('param', 'exp_avg', 'exp_avg_sq')):
        assert torch.equal(a, b), name
    assert not torch.equal(state[0][0], p0)
    # the element-wise form (pointers that are not 16-byte aligned) gives the same bits as well
    big = [torch.zeros(n + 1, device=dev) for _ in range(4)]
    pc, gc, mc, vc = (t[1:] for t in big)
    pc.copy_(p0)
    gen = torch.Generator(device='cpu').manual_seed(21)
    torch.randn(n, generator=gen)
    for step in range(1, 6):
        gc.copy_((torch.randn(n, generator=gen) * 0.1).to(dev))
        _lib().check(lib.sf_adam_flat_groups_f32(pc.data_ptr(), gc.data_ptr(), mc.data_ptr(), vc.data_ptr(), n, step, _groups([(0, 2e-4)]), 1,
                                                 0.9, 0.999, 1e-8, None, _stream()))
    assert torch.equal(pc, state[0][0]) and torch.equal(mc, state[0][1]) and torch.equal(vc, state[0][2])


def _eleven(dev, seed):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(k, generator=gen).to(dev)) for k in SIZES]


def _set_grads(pas, pbs, step, scale):
    gen = torch.Generator(device='cpu').manual_seed(100 + step)
    for pa, pb in zip(pas, pbs):
        gr = (torch.randn(pa.shape, generator=gen) * scale).to(pa.device)
        pa.grad, pb.grad = gr.clone(), gr.clone()


def test_two_groups_match_torch(dev):
    from slotformer_amd import train
    pa, pb = _eleven(dev, 31), _eleven(dev, 31)
    ref = torch.optim.Adam([{'params': pa[:6]}, {'params': pa[6:], 'lr': 3e-4}], lr=2e-4)
    opt = train.FlatAdam([{'params': pb[:6]}, {'params': pb[6:], 'lr': 3e-4}], lr=2e-4)
    assert [g['lr'] for g in opt.param_groups] == [2e-4, 3e-4] and opt.lr == 2e-4
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert opt.params[6].data_ptr() == opt.flat.data_ptr() + 4 * sum(SIZES[:6])   # group 1 begins where group 0 ends
    for step in range(5):
        if step == 2:   # a schedule written for torch.optim assigns to param_groups
            for o in (ref, opt):
                o.param_groups[0]['lr'], o.param_groups[1]['lr'] = 5e-4, 1e-4
        _set_grads(pa, pb, step, 0.1)
        ref.step()
        opt.step()
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert rel_err(y, x.detach().cpu()) < 1e-5, i   # fp32 rounding of the bias corrections
    assert opt.grad_norm is None and opt.clip_grad is None


def test_clipped_step_matches_torch(dev):
    from slotformer_amd import train
    pa, pb = _eleven(dev, 41), _eleven(dev, 41)
    ref = torch.optim.Adam([{'params': pa[:6]}, {'params': pa[6:], 'lr': 3e-4}], lr=2e-4)
    opt = train.FlatAdam([{'params': pb[:6]}, {'params': pb[6:], 'lr': 3e-4}], lr=2e-4, clip_grad=0.05)
    n = sum(SIZES)
    # ||g|| ~ scale * sqrt(n) ~ 80 * scale: steps 0-2 clip (norm ~ 8), steps 3-4 do not (norm ~ 0.008)
    seen = []
    for step, scale in enumerate((0.1, 0.1, 0.1, 1e-4, 1e-4)):
        _set_grads(pa, pb, step, scale)
        before = [p.grad.clone() for p in pb]
        flat = torch.cat([p.grad.reshape(-1) for p in pb])
        tnorm = torch.nn.utils.clip_grad_norm_(pa, 0.05).item()
        ref.step()
        opt.step()
        f64, bar = _bar(flat, tnorm)
        got = opt.grad_norm.item()
        print(f'step {step}: torch norm {tnorm:.9g}  FlatAdam norm {got:.9g}  float64 {f64:.12g}  n={n}')
        seen.append(tnorm > 0.05)
        assert abs(got - f64) / f64 <= bar
        assert opt.grad_nonfinite.item() == 0.
        assert all(torch.equal(p.grad, b) for p, b in zip(pb, before))   # p.grad is left unclipped
    assert seen == [True, True, True, False, False]
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert rel_err(y, x.detach().cpu()) < 1e-5, i


def test_clipped_real_model(dev):
    """SlotRollouter with the gradients of its own backward(): three clipped steps against a twin under torch's clip + Adam,
    then the inference engine must see the stepped weights (the version bump reaches the plan caches).

    The twin takes COPIES of the same gradients instead of differentiating for itself.  The key bias of every attention layer
    (the middle third of in_proj_bias) has a gradient that is zero in exact arithmetic -- softmax does not see a shift of
    all logits of a row -- so what backward() returns there is rounding noise, and Adam, which divides by the gradient's own
    size, turns that noise into steps of the size of the learning rate.  Two models that each run their own backward part
    ways there at the first differing ulp of a parameter, whichever optimiser steps them (fp32 autograd of the oracle on this
    model and batch: |gradient| <= 1.4e-10 on the key third against 4e-3 / 4e-2 on the query / value thirds, and a 1e-7 relative
    change of one weight flips the sign of 76 of its 128 entries while the other thirds move by 3e-7); that says nothing about
    the optimiser.  With the same gradients on both sides the comparison is of the clip and the update alone."""
    from slotformer_amd import train
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(3)
    a = SlotRollouter(**gu.C1_ROLL['rollout_dict']).to(dev)
    b = SlotRollouter(**gu.C1_ROLL['rollout_dict']).to(dev)
    b.load_state_dict(a.state_dict())
    b.train()
    for mod in b.modules():   # no dropout masks: the run is a function of the seeds below alone
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.
    pa = [p for p in a.parameters() if p.requires_grad]
    ref = torch.optim.Adam(pa, lr=2e-4)
    opt = train.FlatAdam(b.parameters(), lr=2e-4, clip_grad=0.05)
    assert len(pa) == len(opt.params)
    x = gu.seeded_normal((2, 6, 6, 128), 5).to(dev)
    tgt = gu.seeded_normal((2, 3, 6, 128), 6).to(dev)
    clipped = []
    for step in range(3):
        opt.zero_grad()
        ((b(x, 3) - tgt)**2).mean().backward()
        for p, q in zip(pa, opt.params):
            p.grad = q.grad.clone()
        tnorm = torch.nn.utils.clip_grad_norm_(pa, 0.05).item()
        ref.step()
        opt.step()
        print(f'step {step}: torch norm {tnorm:.9g}  FlatAdam norm {opt.grad_norm.item():.9g}')
        clipped.append(tnorm > 0.05)
        assert abs(opt.grad_norm.item() - tnorm) <= 1e-6 * tnorm and opt.grad_nonfinite.item() == 0.
    assert all(clipped)   # the clip was at work in every step
    for (n_, x_), y_ in zip(a.named_parameters(), b.parameters()):
        assert rel_err(y_, x_.detach().cpu()) < 1e-5, n_
    with torch.no_grad():
        assert rel_err(b.eval()(x, 3), a.eval()(x, 3).cpu()) < 1e-5


def test_refusals(dev):
    lib = _lib().lib()
    n = 1000
    t = [torch.zeros(n, device=dev) for _ in range(4)]
    before = [x.clone() for x in t]
    t[1].fill_(1.)
    before[1].fill_(1.)
    ptrs = [x.data_ptr() for x in t]

    def adam(groups, num, step=1):
        return lib.sf_adam_flat_groups_f32(*ptrs, n, step, groups, num, 0.9, 0.999, 1e-8, None, _stream())

    def err():
        return lib.sf_last_error_string().decode()

    nine = _groups([(100 * k, 1e-3) for k in range(9)])
    assert adam(nine, 0) < 0 and 'groups' in err()
    assert adam(nine, 9) < 0 and 'groups' in err()
    assert adam(_groups([(4, 1e-3), (8, 1e-3)]), 2) < 0 and 'begins at 0' in err()
    assert adam(_groups([(0, 1e-3), (500, 1e-3), (400, 1e-3)]), 3) < 0 and 'ascend' in err()
    assert adam(_groups([(0, 1e-3), (n + 1, 1e-3)]), 2) < 0 and 'outside' in err()
    assert adam(_groups([(0, 1e-3)]), 1, step=0) < 0 and 'Adam' in err()
    assert lib.sf_adam_flat_groups_f32(None, *ptrs[1:], n, 1, _groups([(0, 1e-3)]), 1, 0.9, 0.999, 1e-8, None, _stream()) < 0
    out = torch.full((3, ), 7., device=dev)
    ws = _ws(n, dev)
    assert lib.sf_grad_clip_coef_f32(ptrs[1], n, 0.05, None, ws.data_ptr(), ws.numel(), _stream()) < 0 and 'null' in err()
    assert lib.sf_grad_clip_coef_f32(ptrs[1], n, 0.05, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, _stream()) < 0 and 'workspace' in err()
    torch.cuda.synchronize()
    # nothing was launched: parameters, moments, the outputs and the workspace are untouched
    assert all(torch.equal(x, y) for x, y in zip(t, before))
    assert torch.equal(out, torch.full((3, ), 7., device=dev)) and not ws.any()
    # and the accepted forms of the same calls go through
    assert adam(_groups([(0, 1e-3), (500, 2e-3)]), 2) == 0
    assert lib.sf_grad_clip_coef_f32(ptrs[1], n, 0.05, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()) == 0
    assert abs(out[0].item() - n**0.5) < 1e-4 and not torch.equal(t[0], before[0])
