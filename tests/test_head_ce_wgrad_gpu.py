"""GPU: the head's own gradient without the logits (sf_head_ce_wgrad_f32 in csrc/head_ce.hip, `train.head_cross_entropy(..., weight_grad=True)`)
and STEVE's training step on it (`STEVE.fused_token_loss`).  The kernel is held to torch.float64 `F.cross_entropy` with autograd on the CPU -- dW,
and dx in the same call -- at L2TOL = 2e-3, the bar tests/test_head_ce_gpu.py uses for dx.  Measured errors: profiles/head_ce_wgrad.md."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle
from test_engine_gpu import build

pytestmark = pytest.mark.gpu

TOL = 1e-3      # loss: relative
L2TOL = 2e-3    # gradients: relative L2 norm


def l2_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def splits(R, V, K):
    """row splits of a launch, read off the workspace the library asks for: it holds one [V, K] block per split"""
    from slotformer_amd import _lib
    return _lib.lib().sf_head_ce_wgrad_workspace_bytes(R, V, K) // (V * K * 4)


def _split_rows():
    """The smallest R < 4096 at which a 64-word head is swept in S > 1 splits of three tiles or more (both staging buffers are reused), the last
    split shorter than the others and the last tile ragged."""
    for R in range(33, 4096):
        tiles, S = -(-R // 32), splits(R, 64, 64)
        per = -(-tiles // S)
        if S > 1 and per >= 3 and tiles - (S - 1) * per < per and R % 32:
            return R
    raise AssertionError('no such R')


# one row (three waves without work); either side of a row tile; three word blocks, the slab part-filled; the widest K; the real head; split rows
SHAPES = [(1, 32, 32), (31, 64, 64), (33, 64, 64), (65, 96, 64), (64, 160, 256), (130, 4096, 192), ('split', 64, 64)]


def _targets(R, V, gen):
    """word 0 and word V - 1 occur, and a whole tile of 32 rows shares one target where there is one"""
    t = torch.randint(0, V, (R, ), generator=gen)
    if R >= 64:
        t[:32] = 7 % V
    t[-1] = 0
    if R >= 2:
        t[0] = V - 1
    return t


def reference(x, w, t, weight=None, g=1.):
    """float64 on the CPU: d(g sum_r weight_r CE_r) / dW and / dx, one autograd call"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(xr @ wr.t(), t, reduction='none')
    (g * (ce if weight is None else ce * weight.double()).sum()).backward()
    assert bool(torch.isfinite(wr.grad).all() and torch.isfinite(xr.grad).all())
    return wr.grad, xr.grad


@functools.lru_cache(maxsize=None)
def case(R, V, K, peak=None):
    """x, w, targets and the float64 reference of the unweighted sum of the rows' losses, computed once and shared.  The logits have a standard
    deviation of about 2; with `peak`, x is scaled so that the largest logit is +-peak."""
    gen = torch.Generator().manual_seed(1000 * R + V + K)
    x = torch.randn(R, K, generator=gen) * 2
    w = torch.randn(V, K, generator=gen) / K**0.5
    if peak is not None:
        x = (x * (peak / (x.double() @ w.double().t()).abs().max())).float()
    t = _targets(R, V, gen)
    dw, dx = reference(x, w, t)
    return dict(x=x, w=w, t=t, dW=dw, dx=dx, peak=float((x.double() @ w.double().t()).abs().max()))


def run(dev, c, dtype=torch.int64, ld=None, ldw=None, g=1., group_w=None, group=1, t=None, out=None):
    """forward, dx and dW launches on case `c` -> dW, dx on the host"""
    from slotformer_amd import ops
    x, t = c['x'], c['t'] if t is None else t
    R, K = x.shape
    V = c['w'].shape[0]
    if ld is None:
        xd = x.to(dev).contiguous()
    else:   # rows of a wider buffer with finite filler between them
        buf = torch.full((R, ld), 1e3, device=dev)
        buf[:, :K] = x.to(dev)
        xd = buf[:, :K]
    if out is None and ldw is not None:   # NaN in the buffer: it is overwritten, and only in its first K columns
        out = torch.full((V, ldw), float('nan'), device=dev)[:, :K]
    packed = ops.pack_head_ce_weight(c['w'].to(dev))
    td = t.to(dev).to(dtype)
    gw = None if group_w is None else group_w.to(dev)
    gd = torch.tensor([g], device=dev)
    lse, _ = ops.head_ce_forward(xd, packed, td, V, gw, group)
    dx = ops.head_ce_backward(xd, packed, td, V, lse, gd, gw, group)
    dW = ops.head_ce_wgrad(xd, packed, td, V, lse, gd, gw, group, out=out)
    assert dW.shape == (V, K)
    return dW.cpu(), dx.cpu()


@pytest.mark.parametrize('dtype', [torch.int64, torch.int16], ids=['i64', 'i16'])
@pytest.mark.parametrize('R,V,K', SHAPES)
def test_wgrad_vs_float64(dev, R, V, K, dtype):
    if R == 'split':
        R = _split_rows()
        assert 32 < R < 4096 and splits(R, V, K) > 1
    c = case(R, V, K)
    dW, dx = run(dev, c, dtype)
    e = (l2_err(dW, c['dW']), l2_err(dx, c['dx']))
    print(f'head_ce_wgrad R {R} V {V} K {K} S {splits(R, V, K)}: dW(l2) {e[0]:.3g} dx(l2) {e[1]:.3g}')
    assert e[0] < L2TOL and e[1] < L2TOL


@pytest.mark.parametrize('R,V,K,group', [(65, 96, 64, 1), (64, 160, 256, 8), (130, 4096, 192, 1), (1, 32, 32, 1)])
def test_strided_rows_scaled_gradient_and_group_weights(dev, R, V, K, group):
    """ld > K, ldw > K, g != 1 and group weights with zeros: dW is the float64 gradient of the kept rows ALONE"""
    c = case(R, V, K)
    gen = torch.Generator().manual_seed(R)
    gw = torch.rand(R // group, generator=gen) + 0.5
    gw[::3] = 0.
    if R == 1:
        gw[:] = 1.5
    g = -0.37
    ldw = K + 5
    out = torch.full((V, ldw), float('nan'), device=dev)
    dW, dx = run(dev, c, ld=K + 12, g=g, group_w=gw, group=group, out=out[:, :K])
    wr = gw.repeat_interleave(group)
    keep = wr != 0
    assert R == 1 or not bool(keep.all())
    want_dw, want_dx = reference(c['x'][keep], c['w'], c['t'][keep], wr[keep], g)
    e = (l2_err(dW, want_dw), l2_err(dx[keep], want_dx))
    print(f'head_ce_wgrad strided R {R} V {V} K {K} group {group}: dW(l2) {e[0]:.3g} dx(l2) {e[1]:.3g}')
    assert e[0] < L2TOL and e[1] < L2TOL
    assert bool(torch.isnan(out[:, K:]).all()) and not bool(torch.isnan(out[:, :K]).any())   # nothing beyond column K is written


def test_logits_of_80_do_not_overflow(dev):
    c = case(63, 64, 64, 80.)
    assert 79.9 < c['peak'] < 80.1
    dW, dx = run(dev, c)
    assert bool(torch.isfinite(dW).all())
    e = (l2_err(dW, c['dW']), l2_err(dx, c['dx']))
    print(f'head_ce_wgrad logits +-80: dW(l2) {e[0]:.3g} dx(l2) {e[1]:.3g}')
    assert e[0] < L2TOL and e[1] < L2TOL


def test_target_outside_the_vocabulary_matches_nothing(dev):
    """picked by comparison, never by address: such a row brings its softmax part alone"""
    c = case(65, 96, 64)
    t = c['t'].clone()
    t[3], t[64] = -1, 96
    p = torch.softmax(c['x'].double() @ c['w'].double().t(), 1)
    valid = (t >= 0) & (t < 96)
    p[valid, t[valid]] -= 1.
    want = p.t() @ c['x'].double()
    for dtype in (torch.int64, torch.int16):
        dW, _ = run(dev, c, dtype, t=t)
        e = l2_err(dW, want)
        print(f'head_ce_wgrad targets -1 and V ({dtype}): dW(l2) {e:.3g}')
        assert e < L2TOL
    assert l2_err(c['dW'], want) > 10 * L2TOL   # the two rows' one-hot terms are visible at this bar


def test_two_calls_give_the_same_bits_and_overwrite(dev):
    from slotformer_amd import ops
    for R, V, K in ((130, 4096, 192), (_split_rows(), 64, 64)):
        c = case(R, V, K)
        gw = torch.ones(R)
        a, _ = run(dev, c, g=0.5, group_w=gw)
        b, _ = run(dev, c, g=0.5, group_w=gw, out=torch.full((V, K), float('nan'), device=dev))
        assert torch.equal(a, b) and not bool(torch.isnan(b).any())
    # the C entry with R = 0 (no tensor of no rows has an address to pass, so the buffers are those of one row): zeros
    from slotformer_amd import _lib
    c = case(31, 64, 64)
    x, lse, g, t = c['x'][:1].to(dev), torch.zeros(1, device=dev), torch.ones(1, device=dev), c['t'][:1].to(dev)
    packed = ops.pack_head_ce_weight(c['w'].to(dev))
    z = torch.full((64, 64), float('nan'), device=dev)
    ws = torch.empty(_lib.lib().sf_head_ce_wgrad_workspace_bytes(0, 64, 64), dtype=torch.uint8, device=dev)
    assert ws.numel() == 64 * 64 * 4
    rc = _lib.lib().sf_head_ce_wgrad_f32(x.data_ptr(), 64, packed.data_ptr(), t.data_ptr(), None, None, lse.data_ptr(), g.data_ptr(), z.data_ptr(), 64,
                                         0, 64, 64, 1, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0 and bool((z == 0).all())


def test_one_node_for_a_trained_and_a_frozen_head(dev):
    from slotformer_amd import train
    c = case(65, 96, 64)
    R, V, K = 65, 96, 64
    head = torch.nn.Linear(K, V, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(c['w'])
    t = c['t'].to(dev)
    x = c['x'].to(dev).requires_grad_(True)
    head.weight.requires_grad_(False)
    for wg in (False, True):   # with a frozen head the keyword changes nothing
        x.grad = None
        l0, _ = train.head_cross_entropy(x, head, t, weight_grad=wg)
        l0.backward()
        frozen = (l0.detach().clone(), x.grad.clone())
        assert head.weight.grad is None
    head.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='weight gradient.*weight_grad=True'):
        train.head_cross_entropy(x, head, t)
    x.grad = None
    l1, stats = train.head_cross_entropy(x, head, t, weight_grad=True)
    l1.backward()
    assert torch.equal(l1.detach(), frozen[0]) and torch.equal(x.grad, frozen[1]) and float(stats[1]) == R
    assert head.weight.grad.shape == (V, K) and head.weight.grad.dtype == torch.float32
    assert l2_err(head.weight.grad, c['dW'] / R) < L2TOL and l2_err(x.grad, c['dx'] / R) < L2TOL
    # x without a gradient: the same dW, no dx
    dw = head.weight.grad.clone()
    head.weight.grad = None
    train.head_cross_entropy(x.detach(), head, t, weight_grad=True)[0].backward()
    assert torch.equal(head.weight.grad, dw)
    # the packed copy follows the optimiser's step
    opt = torch.optim.SGD(head.parameters(), lr=0.5)
    opt.step()
    l2, _ = train.head_cross_entropy(x, head, t, weight_grad=True)
    want = torch.nn.functional.cross_entropy(c['x'].double() @ head.weight.detach().cpu().double().t(), c['t'])
    assert abs(float(l2.detach()) - float(want)) < TOL * float(want)
    assert float(want) < float(l1.detach()) - 1e-3   # (the step did move the weight)


def _peak(dev, fn):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base, out


def test_memory_with_a_trained_head_does_not_grow_with_rows_times_vocabulary(dev):
    """R 8192 x V 4096: one [R, V] float32 tensor is 128 MiB.  Forward + backward through the fused node with a TRAINED head stays below half of
    that (the workspace of eight [V, K] blocks is 24 MiB; dx, dW, the packed head and x add about 21 MiB); the chain it replaces, run here too,
    exceeds 128 MiB, so the bound discriminates."""
    from slotformer_amd import train
    R, V, K = 8192, 4096, 192
    gen = torch.Generator().manual_seed(9)
    head = torch.nn.Linear(K, V, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, K, generator=gen) / K**0.5)
    x0 = (torch.randn(R, K, generator=gen) * 2).to(dev)
    t = torch.randint(0, V, (R, ), generator=gen).to(dev)

    def fused():
        x = x0.clone().requires_grad_(True)
        head.weight.grad = None
        loss, _ = train.head_cross_entropy(x, head, t, weight_grad=True)
        loss.backward()
        return float(loss.detach()), x.grad.cpu(), head.weight.grad.cpu()

    def chain():
        x = x0.clone().requires_grad_(True)
        head.weight.grad = None
        loss = train.token_cross_entropy(train.linear(x, head), t)
        loss.backward()
        return float(loss.detach()), x.grad.cpu(), head.weight.grad.cpu()

    fused_peak, (fl, fdx, fdw) = _peak(dev, fused)
    head.weight.grad = None
    chain_peak, (cl, cdx, cdw) = _peak(dev, chain)
    print(f'head_ce_wgrad memory R {R} V {V} K {K}: fused peak {fused_peak / 2**20:.1f} MiB, chain peak {chain_peak / 2**20:.1f} MiB; '
          f'fused vs chain: dW(l2) {l2_err(fdw, cdw):.3g} dx(l2) {l2_err(fdx, cdx):.3g}')
    assert fused_peak < R * V * 4 // 2
    assert chain_peak > R * V * 4
    # the two forms are the same function (each is held to float64 elsewhere)
    assert abs(fl - cl) < TOL * cl and l2_err(fdx, cdx) < 2 * L2TOL and l2_err(fdw, cdw) < 2 * L2TOL


# ---- STEVE's training step ---------------------------------------------------------------------------------------------------------------------
def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.


def test_steve_training_step_golden_with_fused_token_loss(dev, precision):
    """tests/test_train_gpu.py::test_steve_training_step_golden with the attribute on: the same fixture, the same tolerances, and the head's
    gradient among those held to the oracle's autograd."""
    g = gu.load_golden('steve_train')
    cfg = gu.steve_tokens_cfg()
    m, sd = build(cfg, g, 921, dev)
    m.train()
    _no_dropout(m)
    m.testing = False
    m.fused_token_loss = True
    img = gu.seeded_img(1, 2, 64, seed=922)
    tok = torch.from_numpy(g['target_token_id']).to(dev).unflatten(0, (1, 2))
    data = {'img': img.to(dev), 'token_id': tok}
    out = m(data)
    assert 'pred_token_id' not in out and out['token_hidden'].shape == (2, m.h * m.w, m.trans_decoder.d_model)
    assert out['target_token_id'].shape == (2, m.h * m.w)
    loss = m.calc_train_loss(data, out)['token_recon_loss']
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4 * float(g['loss'])
    names = [str(n) for n in g['grad_names']]
    assert 'trans_decoder.head.weight' in names
    got = dict(m.named_parameters())
    assert sorted(n for n, p in got.items() if p.grad is not None) == sorted(names)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    enc = oracle.steve_encode(img, osd, cfg, training=True)
    oracle.steve_forward_tokens(img, enc['slots'], osd, cfg)['token_recon_loss'].backward()
    tol = {'bf16x3': 1e-2, 'f32': 4e-3}[precision]
    worst = 0.
    for n, norm in zip(names, g['grad_norms']):
        if n == 'slot_attention.project_q.0.bias' or float(norm) == 0.:   # structurally zero gradients (see the test this one mirrors)
            assert got[n].grad.abs().max() < 1e-5, n
            continue
        e = l2_err(got[n].grad, osd[n].grad)
        worst = max(worst, e)
        assert e < tol, n
        assert abs(float(got[n].grad.norm()) - float(norm)) < tol * float(norm), n
    print(f'STEVE fused_token_loss ({precision}): head dW(l2) {l2_err(got["trans_decoder.head.weight"].grad, osd["trans_decoder.head.weight"].grad):.3g}, '
          f'worst gradient (l2) {worst:.3g}')
    # a second model with the attribute off: the logits route, the same loss
    m2, _ = build(cfg, g, 921, dev)
    m2.train()
    _no_dropout(m2)
    m2.testing = False
    out2 = m2(data)
    assert 'pred_token_id' in out2 and 'token_hidden' not in out2
    l2 = m2.calc_train_loss(data, out2)['token_recon_loss']
    assert abs(float(l2.detach()) - float(loss.detach())) < 1e-5 * float(l2.detach())
    # evaluation is untouched by the attribute
    m.eval()
    with torch.no_grad():
        assert 'pred_token_id' in m(data)


def test_steve_training_with_all_dropouts_and_fused_token_loss(dev):
    """tests/test_train_gpu.py::test_steve_training_with_all_dropouts with the attribute on: eight FlatAdam steps bring the evaluation loss down"""
    from slotformer_amd import train
    g = gu.load_golden('steve_train')
    m, sd = build(gu.steve_tokens_cfg(), g, 921, dev)
    m.train()
    m.testing = False
    m.fused_token_loss = True
    assert m.trans_decoder.tf_dec.blocks[0].self_attn.attn_dropout.p > 0
    data = {'img': gu.seeded_img(2, 2, 64, seed=923).to(dev)}
    opt = train.FlatAdam([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    torch.manual_seed(0)

    def eval_loss():   # dropout-free measurement on the inference path
        m.eval()
        with torch.no_grad():
            v = float(m.calc_train_loss(data, m(data))['token_recon_loss'])
        m.train()
        return v

    before, hist = eval_loss(), []
    for _ in range(8):
        opt.zero_grad()
        out = m(data)
        assert 'token_hidden' in out
        loss = m.calc_train_loss(data, out)['token_recon_loss']
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    after = eval_loss()
    assert all(np.isfinite(hist)) and after < before - 1e-3, (before, after, hist)
