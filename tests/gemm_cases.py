"""Case tables, float64 references and bounds of the fused GEMM core (csrc/gemm.hip) through its four C entry points -- sf_linear_f32 at every tile
configuration the host rule can pick and every K tail, sf_conv2d_nhwc_f32 off the halo kernel's shape, sf_conv2d_nchw_in_f32 on the scalar loader and
sf_conv_transpose2d_nhwc_f32 -- shared by tests/test_gemm_cases.py (CPU) and tests/test_gemm_gpu.py.  Plain torch on the CPU; the library is not
imported here.

Every reference is computed in float64 from the float32 inputs the kernel gets; the cached ones must not be written into.  Each can also be
evaluated in the arithmetic of the kernels' matrix products (encode_kernel_cases.product: 'split' = hi.hi + hi.lo + lo.hi on bf16 hi / lo operands,
'single' = hi.hi alone, 'f32'), which is what says whether a bound can tell the library's arithmetic modes apart (tests/test_gemm_cases.py).
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from encode_kernel_cases import err_over_bound, product, rnd  # noqa: F401  (re-exported for the two test files)

# per-launch bounds |a - b| <= rtol |b| + floor max |b|: those of tests/test_train_kernels_gpu.py (TOL, TOL_BF16), restated as in
# tests/savi_train_kernel_cases.py because this file does not import a GPU test module; the CPU test holds the copies together
TOL = {'f32': (2e-5, 2e-5), 'bf16x3': (1e-4, 1e-4)}
TOL_BF16 = (2**-6, 2**-6)
PROJECT = {'f32': TOL['f32'], 'bf16x3': TOL['bf16x3'], 'bf16': TOL_BF16}
PRECISION_MODE = {'f32': 0, 'bf16x3': 1, 'bf16': 2}     # sf_set_precision

# The ids sf_linear_config can return: the cases of the switch in launch_by_id (csrc/gemm.hip) minus the ones no default path reaches -- 100, 102,
# 103, 105, 121, 123, 130 (tuning only, SF_DBG=gemmcfg) and 28 (the convolutions' exact-f32 tile, never a linear's).
DEFAULT_IDS_SPLIT = frozenset({106, 107, 108, 109, 115, 122, 131, 132, 133})      # precision 1 and 2
DEFAULT_IDS_F32 = frozenset({1, 3, 4, 7, 31})                                     # precision 0

# (M, N, K) -> (split-bf16 id, exact-f32 id): the smallest shapes that reach each default configuration, with every K tail its loop can end on
LINEAR_CASES = {
    (1, 1, 4): (106, 3),              # one row, one column, one k-quad
    (33, 65, 36): (106, 3),           # ragged everything, tail of 4
    (100, 36, 100): (106, 3),
    (7, 128, 260): (106, 3),          # nk = 3, tail of 4
    (4065, 72, 68): (109, 4),         # the 32x64 f32 tile
    (70, 40, 512): (115, 7),          # BKT 256 with 8-way split-K; in f32 PD == 2 with nk = 4
    (70, 40, 516): (115, 7),          # ... nk = 5
    (70, 40, 644): (115, 7),          # ... nk = 6
    (7, 40, 516): (115, 7),
    (33, 33, 512): (115, 7),
    (520, 40, 516): (109, 7),         # nk = 5 on a double-buffered tile
    (520, 40, 36): (109, 3),          # nk = 1 on a double-buffered tile
    (1210, 1000, 36): (122, 4),       # preload-all with 1 chunk
    (1210, 1000, 68): (122, 4),       # 2
    (1210, 1000, 132): (122, 4),      # 3
    (1210, 1000, 200): (122, 4),      # 4 with a tail
    (1210, 1000, 256): (122, 4),      # 4 exact
    (1210, 1000, 260): (107, 4),
    (1210, 1000, 324): (107, 4),
    (1210, 700, 4): (108, 4),         # 2-way split-K, nk = 1
    (1210, 700, 132): (108, 4),       # nk = 2
    (1210, 700, 260): (108, 4),       # nk = 3
    (49100, 40, 36): (133, 1),        # single-buffered 128x64, ragged last row tile
    (16300, 257, 36): (133, 31),      # N one past two column tiles
    (16300, 384, 36): (131, 31),      # N a multiple of 128
    (12200, 520, 68): (131, 31),      # N >= 512 and not a multiple
    (12200, 520, 132): (131, 31),
    (3044, 1000, 2048): (132, 1),     # long K
    (3044, 1000, 2052): (132, 1),
}
LINEAR_SHAPES = list(LINEAR_CASES)

# mode -> (bias, relu, residual, LayerNorm prologue)
MODES = {
    'plain': (False, False, False, False),
    'bias': (True, False, False, False),
    'bias_relu': (True, True, False, False),
    'residual': (False, False, True, False),
    'ln_bias_relu_residual': (True, True, True, True),
    'ln_only': (False, False, False, True),
}
MODES_BIG = ('plain', 'ln_bias_relu_residual')      # more than 10,000 rows; also all that single-pass bf16 runs
LN_EPS = 1e-5


def modes_of(shape):
    return MODES_BIG if shape[0] > 10000 else tuple(MODES)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0xffffff


@functools.lru_cache(maxsize=2)
def linear_inputs(shape):
    """x [M,K] ~ N(0,1), w [N,K] ~ N(0, 1/K), bias [N], gamma / beta [K], residual [M,N]"""
    M, N, K = shape
    s = _seed('linear3', shape)    # (the third stream tried: under it the only output of (1, 1, 4) is positive before the ReLU, with and without LayerNorm)
    return dict(x=rnd(M, K, seed=s), w=rnd(N, K, seed=s + 1, scale=K**-0.5), b=rnd(N, seed=s + 2, scale=0.1), g=1 + 0.1 * rnd(K, seed=s + 3),
                be=0.1 * rnd(K, seed=s + 4), r=rnd(M, N, seed=s + 5))


def layer_norm64(x, g, be, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean)**2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g.double() + be.double()


def linear_raw(x, w, g, be, eps, arith):
    """LN?(x) . w^T, float64 [M,N].  arith 'f64': no rounding anywhere; any other: the LayerNorm output rounded to float32 (what the kernel stages)
    and the product in that arithmetic"""
    a = x if g is None else layer_norm64(x, g, be, eps)
    if arith == 'f64':
        return a.double() @ w.double().t()
    return product(lambda p, q: p @ q.t(), a.float(), w, arith)


def linear_finish(raw, bias, relu, res):
    out = raw if bias is None else raw + bias.double()
    if relu:
        out = torch.relu(out)
    return out if res is None else out + res.double()


@functools.lru_cache(maxsize=4)
def _linear_raw_cached(shape, ln):
    c = linear_inputs(shape)
    return linear_raw(c['x'], c['w'], c['g'] if ln else None, c['be'], LN_EPS, 'f64')


def linear_eval(shape, mode, arith='f64'):
    """the case's expected output [M,N] in float64 ('f64': cached per (shape, LayerNorm) across modes) or in a kernel's arithmetic"""
    bias, relu, res, ln = MODES[mode]
    c = linear_inputs(shape)
    raw = _linear_raw_cached(shape, ln) if arith == 'f64' else linear_raw(c['x'], c['w'], c['g'] if ln else None, c['be'], LN_EPS, arith)
    return linear_finish(raw, c['b'] if bias else None, relu, c['r'] if res else None)


# ---------------------------------------------------------------------------------------------------------------------
# convolutions: the references are sums over taps of matrix products, so that `product` can evaluate them in a kernel's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def conv_closed(x, w, stride, arith='f64'):
    """Conv2d(ks, stride, padding ks // 2): x [F,H,W,Cin] NHWC, w [Cout,Cin,ks,ks] (torch) -> float64 [F,Ho,Wo,Cout]"""
    F_, H, W, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[2]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    out = torch.zeros(F_ * Ho * Wo, Cout, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :].reshape(-1, Cin)
            out += product(lambda p, q: p @ q.t(), xs, w[:, :, ky, kx], arith)
    return out.view(F_, Ho, Wo, Cout)


def deconv_closed(x, w, stride, arith='f64'):
    """ConvTranspose2d(ks, stride, padding ks // 2, output_padding stride - 1): x [F,H,W,Cin] NHWC, w [Cin,Cout,ks,ks] (torch) -> float64
    [F,H s,W s,Cout]: input pixel (iy, ix) adds x . w[:, :, ky, kx] to output (iy s - pad + ky, ix s - pad + kx)"""
    F_, H, W, Cin = x.shape
    Cout, ks = w.shape[1], w.shape[2]
    pad, Ho, Wo = ks // 2, H * stride, W * stride
    out = torch.zeros(F_, Ho, Wo, Cout, dtype=torch.float64)

    def span(k, n_in, n_out):   # the inputs i with 0 <= i s - pad + k < n_out, and the first output they reach
        lo = max(0, -(-(pad - k) // stride))
        hi = min(n_in - 1, (n_out - 1 + pad - k) // stride)
        return lo, hi, lo * stride - pad + k

    for ky in range(ks):
        for kx in range(ks):
            y0, y1, oy = span(ky, H, Ho)
            x0, x1, ox = span(kx, W, Wo)
            if y1 < y0 or x1 < x0:
                continue
            p = product(lambda a, b: a @ b, x.reshape(-1, Cin), w[:, :, ky, kx], arith).view(F_, H, W, Cout)
            out[:, oy:oy + stride * (y1 - y0) + 1:stride, ox:ox + stride * (x1 - x0) + 1:stride] += p[:, y0:y1 + 1, x0:x1 + 1]
    return out


def conv_finish(raw, bias, relu, table):
    """bias, ReLU, then the [Ho*Wo, Cout] table added to every frame, in float64"""
    out = raw if bias is None else raw + bias.double()
    if relu:
        out = torch.relu(out)
    return out if table is None else out + table.double().view(1, *raw.shape[1:])


# sf_conv2d_nhwc_f32 off the halo kernel's shape: (F, H, W, Cin, Cout, ks)
NHWC_CASES = [
    (3, 6, 10, 8, 20, 3),         # K = 72, generic index arithmetic
    (2, 5, 7, 64, 64, 5),         # the constant-folded Cin == 64 && ks == 5 branch at a width that is not 64
    (5, 12, 17, 4, 36, 5),        # 1020 rows = eight row tiles: the XCD tile remap
    (2, 6, 10, 8, 20, 1),
]
NHWC_OPTIONS = [(relu, bias, table) for relu in (0, 1) for bias in (False, True) for table in (False, True)]
# sf_conv2d_nchw_in_f32 on the generic (scalar) loader: (F, Cin, Hin, Win, Cout, ks, stride)
NCHW_CASES = [
    (2, 3, 12, 20, 24, 5, 1),
    (2, 3, 12, 20, 24, 5, 2),
    (3, 1, 9, 14, 8, 3, 1),       # K = 9
    (1, 3, 64, 64, 64, 5, 1),     # precision 0 only: there it is the GEMM and not csrc/conv_first.hip
]
NCHW_F32_ONLY = (1, 3, 64, 64, 64, 5, 1)
NCHW_GAP = 7                      # floats of NaN between two frames (frame_stride = Cin Hin Win + NCHW_GAP)
# sf_conv_transpose2d_nhwc_f32: (F, Hin, Win, Cin, Cout, ks, stride)
DECONV_CASES = [
    (2, 3, 5, 8, 12, 5, 2),
    (2, 4, 7, 64, 20, 3, 2),
    (2, 5, 3, 8, 12, 5, 1),       # the single-launch gather
    (2, 3, 4, 8, 12, 5, 3),       # three-by-three parity classes
]


@functools.lru_cache(maxsize=None)
def nhwc_case(case):
    F_, H, W, Cin, Cout, ks = case
    s = _seed('nhwc', case)
    x, w = rnd(F_, H, W, Cin, seed=s), rnd(Cout, Cin, ks, ks, seed=s + 1, scale=(ks * ks * Cin)**-0.5)
    return dict(x=x, w=w, b=rnd(Cout, seed=s + 2, scale=0.1), table=rnd(H * W, Cout, seed=s + 3), raw=conv_closed(x, w, 1))


@functools.lru_cache(maxsize=None)
def nchw_case(case):
    """img is NCHW [F,Cin,Hin,Win]; the references take it as NHWC"""
    F_, Cin, Hin, Win, Cout, ks, stride = case
    s = _seed('nchw', case)
    img, w = rnd(F_, Cin, Hin, Win, seed=s), rnd(Cout, Cin, ks, ks, seed=s + 1, scale=(ks * ks * Cin)**-0.5)
    raw = conv_closed(img.permute(0, 2, 3, 1).contiguous(), w, stride)
    return dict(img=img, w=w, b=rnd(Cout, seed=s + 2, scale=0.1), table=rnd(raw.shape[1] * raw.shape[2], Cout, seed=s + 3), raw=raw)


@functools.lru_cache(maxsize=None)
def deconv_case(case):
    F_, H, W, Cin, Cout, ks, stride = case
    s = _seed('deconv', case)
    x, w = rnd(F_, H, W, Cin, seed=s), rnd(Cin, Cout, ks, ks, seed=s + 1, scale=2 * (ks * ks * Cin)**-0.5)
    return dict(x=x, w=w, b=rnd(Cout, seed=s + 2, scale=0.1), raw=deconv_closed(x, w, stride))
