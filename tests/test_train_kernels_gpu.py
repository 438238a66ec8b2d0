"""GPU parity of the training building blocks of rollout_train.hip against torch autograd in float64
on the CPU, one library call at a time, at the shapes where the host code picks a different branch.

Every comparison is element by element in the allclose form of test_engine_gpu.elementwise_close:
|a - b| <= rtol |b| + floor max|b|.  The bounds per precision mode are those of test_kernels_gpu.tol.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {'f32': (2e-5, 2e-5), 'bf16x3': (1e-4, 1e-4)}
TOL_BF16 = (2**-6, 2**-6)   # precision mode 2: one bf16 product per pair, 8 mantissa bits per operand
LDS_MAX = 160 * 1024        # the LDS of one CU


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def close(a, b, tol, what):
    """assert |a - b| <= rtol |b| + floor max|b| element by element; returns the largest error over its bound"""
    rtol, floor = tol
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bound = rtol * b.abs() + floor * b.abs().max()
    ratio = ((a - b).abs() / bound.clamp_min(1e-300)).max().item()
    print(f'{what}: max err / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: max err / bound {ratio:.3f}'
    return ratio


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# sf_linear_bwd_f32: weight gradient (grad_gemm_tn_kernel over tn_splits row splits, reduce_partials[_wide]_kernel),
# bias column sums, data gradient
# ---------------------------------------------------------------------------------------------------------------------
def _linear_ref(x, w, b, dy, mask):
    """float64 autograd of y = act(x W^T + b); the ReLU takes the GPU forward's branch (mask = y_gpu > 0), so an entry
    within rounding distance of the kink cannot make the two sides differ by a whole sample's contribution"""
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    y = F.linear(x64, w64, b64)
    if mask is not None:
        y = torch.where(mask, y, torch.zeros_like(y))
    y.backward(dy.double())
    return x64.grad, w64.grad, (b64.grad if b is not None else None)


LINEAR_SHAPES = [
    (7, 64, 64),          # M <= 64: one split, the kernel writes dW directly
    (64, 256, 256),       # one split, 16 tiles
    (1060, 768, 256),     # 11 splits of 128 rows: splits 9 and 10 start past the last row (empty partials)
    (1000, 64, 64),       # 16 splits of 64 rows, the last one with a ragged 40-row tail (chunk of 32 + 8)
    (49152, 64, 64),      # 512 splits: reduce_partials_wide_kernel (G >= 32)
    (49157, 192, 192),    # 57 splits, ragged: reduce_partials_wide_kernel
    (1344, 1024, 256),    # 8 splits: reduce_partials_kernel (C2's in-projection rows)
    (1344, 768, 256),     # 11 splits: reduce_partials_kernel
    (50000, 576, 192),    # training size: 19 splits, wide reduction, bias over three column blocks
]


# every (relu, bias) pair on the small shapes; on the big ones the two mixed pairs, which still take each branch both ways
LINEAR_CASES = [(M, N, K, relu, bias) for M, N, K in LINEAR_SHAPES
                for relu, bias in ([(False, True), (True, False)] + ([(True, True), (False, False)] if M <= 2000 else []))]


@pytest.mark.parametrize('M,N,K,relu,bias', LINEAR_CASES)
def test_linear_bwd(dev, precision, M, N, K, relu, bias):
    """train._Linear forward + backward: dx, dW, db against float64 autograd."""
    from slotformer_amd import train
    x, w, dy = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K**-0.5), rnd(M, N, seed=3)
    b = rnd(N, seed=4, scale=0.1) if bias else None
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if bias else None
    y = train._Linear.apply(xg, wg, bg, relu)
    y.backward(dy.to(dev))
    mask = (y.detach().cpu() > 0) if relu else None
    rx, rw, rb = _linear_ref(x, w, b, dy, mask)
    tol = TOL[precision]
    close(wg.grad, rw, tol, 'dW')
    close(xg.grad, rx, tol, 'dx')
    if bias:
        close(bg.grad, rb, tol, 'db')


def _linear_bwd_call(x, w, y, dy, dx, dW, db, relu):
    M, K = x.shape
    N = w.shape[0]
    nb = _lib().sf_linear_bwd_workspace_bytes(M, N, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    return _lib().sf_linear_bwd_f32(_p(x), _p(w), _p(y), _p(dy), _p(dx), _p(dW), _p(db), M, N, K, int(relu), ws.data_ptr(), nb,
                                    _stream())


@pytest.mark.parametrize('M,N,K', [(1000, 64, 64), (1344, 768, 256), (49157, 192, 192)])
def test_linear_bwd_relu_mask_null_and_unaligned_destinations(dev, precision, M, N, K):
    """Direct ABI calls for the forms the autograd nodes never produce: the ReLU masks dy in place exactly where y > 0;
    dx = NULL and db = NULL leave dW bit-identical; dW and db as views at odd float offsets of one flat buffer."""
    x, w, dy = rnd(M, K, seed=11), rnd(N, K, seed=12, scale=K**-0.5), rnd(M, N, seed=13)
    b = rnd(N, seed=14, scale=0.1)
    xd, wd = x.to(dev), w.to(dev)
    y = F.linear(xd, wd, b.to(dev))   # any forward output: only its sign is read
    d0 = dy.to(dev)
    dx, dW, db = torch.empty(M, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    assert _linear_bwd_call(xd, wd, y, d0, dx, dW, db, True) == 0
    mask = y.cpu() > 0
    assert torch.equal(d0.cpu(), torch.where(mask, dy, torch.zeros_like(dy)))   # masked in place, bit for bit
    rx, rw, rb = _linear_ref(x, w, b, dy, mask)
    tol = TOL[precision]
    close(dW, rw, tol, 'dW')
    close(dx, rx, tol, 'dx')
    close(db, rb, tol, 'db')
    # dx = NULL, db = NULL: the same dW
    dW2 = torch.full((N, K), float('nan'), device=dev)
    assert _linear_bwd_call(xd, wd, None, d0.clone(), None, dW2, None, False) == 0
    assert torch.equal(dW2, dW)
    # unaligned destinations: dW at float offset 1, db right behind it, NaN guards on both ends stay untouched
    flat = torch.full((1 + N * K + N + 1, ), float('nan'), device=dev)
    fW, fb = flat[1:1 + N * K].view(N, K), flat[1 + N * K:1 + N * K + N]
    assert fW.data_ptr() % 16 != 0 and fb.data_ptr() % 16 != 0
    assert _linear_bwd_call(xd, wd, None, d0.clone(), None, fW, fb, False) == 0
    assert torch.equal(fW, dW) and torch.equal(fb, db)
    assert torch.isnan(flat[0]) and torch.isnan(flat[-1])


def test_linear_bwd_single_pass_bf16(dev):
    """Precision mode 2 (grad_gemm_tn_kernel<2>, hi * hi only) with a bf16-sized bound."""
    from slotformer_amd import train
    lib = _lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(2)
    try:
        M, N, K = 1344, 768, 256
        x, w, dy, b = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=K**-0.5), rnd(M, N, seed=23), rnd(N, seed=24, scale=0.1)
        xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
        train._Linear.apply(xg, wg, bg, False).backward(dy.to(dev))
        rx, rw, rb = _linear_ref(x, w, b, dy, None)
        close(wg.grad, rw, TOL_BF16, 'dW')
        close(xg.grad, rx, TOL_BF16, 'dx')
        close(bg.grad, rb, TOL['f32'], 'db')   # column sums are fp32 in every mode
        # and mode 2 is really the single-pass product: well outside the split-bf16 bound
        assert (wg.grad.cpu().double() - rw).abs().max().item() > TOL['bf16x3'][1] * rw.abs().max().item()
    finally:
        lib.sf_set_precision(old)


@pytest.mark.parametrize('n', [64,     # 64 columns x 4 row lanes per workgroup
                               192,    # one 256-lane block with 64 idle columns
                               576,    # three column blocks
                               1024])
@pytest.mark.parametrize('rows', [1,       # one group, one row
                                  127,     # one group: reduce_partials_kernel with G = 1
                                  129,     # two groups of 65
                                  65537])  # the group count clamps at 512 (509 groups of 129): reduce_partials_wide_kernel
def test_bias_column_sums(dev, precision, n, rows):
    """grad_bias (colsum_partial_kernel + split reduction) through sf_linear_bwd_f32 with a bias."""
    K = 64
    x, w, dy = rnd(rows, K, seed=31), rnd(n, K, seed=32, scale=0.1), rnd(rows, n, seed=33)
    db = torch.full((n, ), float('nan'), device=dev)
    dW = torch.empty(n, K, device=dev)
    assert _linear_bwd_call(x.to(dev), w.to(dev), None, dy.to(dev), None, dW, db, False) == 0
    close(db, dy.double().sum(0), TOL[precision], 'db')


# ---------------------------------------------------------------------------------------------------------------------
# sf_layernorm_bwd_f32: ln_param_partial_kernel + split reduction (dgamma, dbeta), ln_bwd_kernel (dx)
# ---------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, g, b, dy, eps=1e-5):
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    F.layer_norm(x64, (x.shape[-1], ), g64, b64, eps).backward(dy.double())
    return x64.grad, g64.grad, b64.grad


@pytest.mark.parametrize('D', [4, 64, 192, 256, 260, 1020, 1024])   # 1 .. 256 float4 columns per lane set; 260 / 1020: ragged last float4 pass
@pytest.mark.parametrize('rows', [1, 3,     # fewer rows than the 4 waves of a group
                                  65,       # two groups (64 + 1 rows)
                                  4097,     # 65 groups of 64 (+1): reduce_partials_wide_kernel
                                  40000])   # 507 groups of 79 rows (not a multiple of the 4 waves)
def test_layernorm_bwd(dev, precision, D, rows):
    """train._LayerNorm forward + backward: dx, dgamma, dbeta against float64 autograd."""
    from slotformer_amd import train
    x, dy = rnd(rows, D, seed=41), rnd(rows, D, seed=42)
    g, b = 1 + 0.1 * rnd(D, seed=43), 0.1 * rnd(D, seed=44)
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, g, b))
    train._LayerNorm.apply(xg, gg, bg, 1e-5).backward(dy.to(dev))
    rx, rg, rb = _ln_ref(x, g, b, dy)
    tol = TOL[precision]
    close(xg.grad, rx, tol, 'dx')
    close(gg.grad, rg, tol, 'dgamma')
    close(bg.grad, rb, tol, 'dbeta')


@pytest.mark.parametrize('D,rows', [(64, 4097), (256, 1344), (1024, 40000)])
def test_layernorm_bwd_large_offset(dev, precision, D, rows):
    """Inputs with a common offset of 1e3 and unit spread: the kernels centre each row before they square it.  The inputs
    themselves resolve only 1e3 * 2^-24 = 6e-5 of the unit spread, and the fp32 row mean carries an error of that order,
    which moves x-hat by as much: the floor is 4 such steps."""
    from slotformer_amd import train
    x, dy = 1e3 + rnd(rows, D, seed=51), rnd(rows, D, seed=52)
    g, b = 1 + 0.1 * rnd(D, seed=53), 0.1 * rnd(D, seed=54)
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, g, b))
    train._LayerNorm.apply(xg, gg, bg, 1e-5).backward(dy.to(dev))
    rx, rg, rb = _ln_ref(x, g, b, dy)
    rtol, floor = TOL[precision]
    tol = (rtol, max(floor, 4 * 1e3 * 2**-24))
    close(xg.grad, rx, tol, 'dx')
    close(gg.grad, rg, tol, 'dgamma')
    close(bg.grad, rb, TOL[precision], 'dbeta')   # a plain column sum of dy: the offset does not enter


@pytest.mark.parametrize('D,rows', [(64, 4097), (260, 65), (1024, 40000)])
def test_layernorm_bwd_flat_bucket(dev, precision, D, rows):
    """dgamma and dbeta as views at an odd float offset of one flat buffer: grad_ln reduces into scratch and copies both
    out with hipMemcpyAsync.  The same bits as aligned destinations; the NaN guards around them stay untouched."""
    x, dy = rnd(rows, D, seed=61), rnd(rows, D, seed=62)
    g = 1 + 0.1 * rnd(D, seed=63)
    xd, dyd, gd = x.to(dev), dy.to(dev), g.to(dev)
    lib = _lib()
    nb = lib.sf_layernorm_bwd_workspace_bytes(D)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def call(dgamma, dbeta):
        dx = torch.empty_like(xd)
        assert lib.sf_layernorm_bwd_f32(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                        rows, D, 1e-5, ws.data_ptr(), nb, _stream()) == 0
        return dx

    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    dx = call(dg, db)
    flat = torch.full((1 + 2 * D + 1, ), float('nan'), device=dev)
    fg, fb = flat[1:1 + D], flat[1 + D:1 + 2 * D]
    assert fg.data_ptr() % 16 != 0
    dx2 = call(fg, fb)
    assert torch.equal(fg, dg) and torch.equal(fb, db) and torch.equal(dx2, dx)
    assert torch.isnan(flat[0]) and torch.isnan(flat[-1])
    rx, rg, rb = _ln_ref(x, g, torch.zeros(D), dy)
    tol = TOL[precision]
    close(fg, rg, tol, 'dgamma')
    close(fb, rb, tol, 'dbeta')
    close(dx2, rx, tol, 'dx')


def test_layernorm_bwd_refuses_bad_widths(dev):
    """Widths the kernels do not handle are refused on the host, before the parameter-gradient launch."""
    lib = _lib()
    buf = torch.zeros(4 * 1028, device=dev)
    for D in (0, 6, 1028):
        nb = lib.sf_layernorm_bwd_workspace_bytes(max(D, 4))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        p = buf.data_ptr()
        assert lib.sf_layernorm_bwd_f32(p, p, p, p, p, p, 1, D, 1e-5, ws.data_ptr(), nb, _stream()) != 0, D
        assert 'LayerNorm width' in lib.sf_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------------
# sf_mha_train_fwd_f32 / sf_mha_train_bwd_f32: attn_train_{fwd,bwd}[_mfma]_kernel
# ---------------------------------------------------------------------------------------------------------------------
def mha_lds_bytes(L, hd):
    """the backward kernel's dynamic LDS (it needs more than the forward): the MFMA kernels (head dim 32 / 64, L <= 96)
    pad L to a multiple of 32, the scalar kernels do not"""
    lp = (L + 31) // 32 * 32 if hd in (32, 64) and L <= 96 else L
    return (4 * lp * (hd + 1) + 2 * lp * (lp + 1)) * 4


def mha_accepts(L, hd):
    return 1 <= L <= 128 and 1 <= hd <= 64 and mha_lds_bytes(L, hd) <= LDS_MAX


def _mha_ref(qkv, dctx, B, L, d, H, p, seed):
    from slotformer_amd.train import dropout_keep_mask
    qo = qkv.double().requires_grad_(True)
    q, k, v = (t.view(B, L, H, d // H).transpose(1, 2) for t in qo.chunk(3, -1))
    att = torch.softmax((q * (d // H)**-0.5) @ k.transpose(-1, -2), dim=-1)
    if p > 0:
        keep = torch.from_numpy(dropout_keep_mask(seed, 0, 0, 0, att.numel(), p).astype(np.float64)).view(att.shape)
        att = att * keep / (1.0 - float(np.float32(p)))
    ctx = (att @ v).transpose(1, 2).reshape(B * L, d)
    ctx.backward(dctx.double())
    return ctx.detach(), qo.grad


def _mha_case(dev, precision, B, L, hd, H, p):
    from slotformer_amd import train
    assert mha_accepts(L, hd)
    d, seed = hd * H, 0x5eed_0000_1234 + L
    qkv, dctx = rnd(B * L, 3 * d, seed=L), rnd(B * L, d, seed=L + 1000)
    qg = qkv.to(dev).requires_grad_(True)
    ctx = train._MHA.apply(qg, B, L, d, H, p, seed)
    ctx.backward(dctx.to(dev))
    rc, rq = _mha_ref(qkv, dctx, B, L, d, H, p, seed)
    tol = TOL[precision]
    close(ctx, rc, tol, 'ctx')
    close(qg.grad, rq, tol, 'dqkv')


@pytest.mark.parametrize('L', [1, 7, 31, 32, 33, 42, 64])   # Lp = 32 / 64 tiles, L = 1 and Lp - 1 / Lp / Lp + 1 edges
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_mha_mfma(dev, precision, L, hd, p):
    """attn_train_{fwd,bwd}_mfma_kernel<hd>; head dim 64 stops at L = 64 (beyond, its backward tile does not fit)."""
    _mha_case(dev, precision, 3, L, hd, 8 if hd == 32 else 4, p)


@pytest.mark.parametrize('L', [90, 96])   # Lp = 96: the reference's Physion window (15 x 6 tokens), 3 x 3 tiles, set_lds past 64 KB
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_mha_mfma_long_window(dev, precision, L, p):
    _mha_case(dev, precision, 3, L, 32, 8, p)


@pytest.mark.parametrize('B,L,hd', [(1, 42, 32), (64, 90, 32), (64, 33, 64), (1, 97, 48), (64, 42, 16)])
def test_mha_batch(dev, precision, B, L, hd):
    """one video and 64 videos per launch (grid (heads, B); dropout index base (b * H + h) L^2)"""
    _mha_case(dev, precision, B, L, hd, 4, 0.1)


@pytest.mark.parametrize('L', [1, 7, 42, 97])   # small, mid, and past the MFMA kernels' 96
@pytest.mark.parametrize('hd', [16, 48])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_mha_scalar(dev, precision, L, hd, p):
    """attn_train_{fwd,bwd}_kernel: head dims the MFMA kernels do not take (hd 48 at L = 97 needs 152 KB of LDS)"""
    _mha_case(dev, precision, 3, L, hd, 4, p)


LMAX = {hd: max(L for L in range(1, 129) if mha_accepts(L, hd)) for hd in (8, 16, 24, 32, 48, 64)}


@pytest.mark.parametrize('hd', sorted(LMAX))
def test_mha_largest_accepted_window(dev, precision, hd):
    """the largest L the ABI accepts per head dim (128 for hd 8; 126, 119, 113, 101 on the scalar kernels past 64 KB of
    LDS; 64 for hd 64 on the MFMA kernel at 97.5 KB)"""
    _mha_case(dev, precision, 2, LMAX[hd], hd, 2, 0.1)


REFUSED = [(129, 8), (0, 32), (127, 16), (120, 24), (114, 32), (102, 48), (65, 64), (90, 64), (96, 64), (97, 64), (128, 64),
           (1, 65)]


@pytest.mark.parametrize('L,hd', REFUSED)
def test_mha_refuses_shapes_that_do_not_fit(dev, L, hd):
    """Shapes outside the accepted range are refused by the host-side checks of both calls, before any launch (the
    buffers are sized for the shape all the same)."""
    assert not mha_accepts(L, hd)
    lib = _lib()
    B, H = 1, 1
    d = hd * H
    qkv = torch.zeros(max(L, 1) * 3 * d, device=dev)
    ctx = torch.zeros(max(L, 1) * d, device=dev)
    dqkv = torch.zeros_like(qkv)
    for p in (0.0, 0.1):
        assert lib.sf_mha_train_fwd_f32(qkv.data_ptr(), ctx.data_ptr(), B, L, d, H, p, 1, _stream()) != 0
        assert 'invalid argument' in lib.sf_last_error_string().decode()
        assert lib.sf_mha_train_bwd_f32(qkv.data_ptr(), ctx.data_ptr(), dqkv.data_ptr(), B, L, d, H, p, 1, _stream()) != 0
        msg = lib.sf_last_error_string().decode()
        assert 'invalid argument' in msg
        if 1 <= L <= 128 and hd <= 64:
            assert '160 KB' in msg, msg
    torch.cuda.synchronize()
    assert not dqkv.any() and not ctx.any()
