"""Case tables, float64 references and bounds of the launches behind SAVi's two convolutional backward passes (csrc/savi_features_train.hip,
csrc/savi_decode_train.hip) -- the 5 x 5 weight gradient (conv_wgrad_kernel, conv_wgrad_win_kernel, reduce_to_oihw_kernel), the masked data-gradient
convolution in its three implementations (csrc/conv_rows4.hip, csrc/conv_halo.hip, the implicit-GEMM epilogue of csrc/gemm.hip), conv0's weight gradient
against the image patches, the position-embedding gradients and the head block of the decoder -- shared by tests/test_savi_train_kernel_cases.py (CPU)
and tests/test_savi_train_kernels_gpu.py.  Plain torch on the CPU; the library is not imported here.

Every reference is computed in float64 from the float32 inputs the kernel gets, once per case (lru_cache): do not write into one.  Each exists twice:
as float64 autograd of F.conv2d / F.conv_transpose2d, and as a closed form (a sum over taps of matrix products), held to 1e-12 of each other by the CPU
test.  The closed form can also be evaluated in the arithmetic of the kernels' matrix products (encode_kernel_cases.product: 'split' = hi.hi + hi.lo +
lo.hi on bf16 hi / lo operands, 'single' = hi.hi alone), which is what says whether a bound can tell the two apart.

Arithmetic modes of the library (sf_set_precision): 0 adds the lo.lo term to the split product, 1 (the default) drops it, 2 is the single product.  Modes 0
and 1 differ by about 2^-18 of a product and CANNOT be told apart by accuracy against float64 at any bound a kernel can meet; nothing here pretends to.
What the bounds do see is mode 1 or 0 running the single-product kernel (2^-9 per operand).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from encode_kernel_cases import err_over_bound, product, rnd  # noqa: F401  (re-exported for the two test files)

# per-launch bounds |a - b| <= rtol |b| + floor max |b|: those of tests/test_train_kernels_gpu.py (TOL, TOL_BF16), restated here because this file does not
# import a GPU test module; the CPU test holds the two copies together
TOL = {'f32': (2e-5, 2e-5), 'bf16x3': (1e-4, 1e-4)}
TOL_BF16 = (2**-6, 2**-6)
KS, CX = 5, 64                      # the kernels are 5 x 5 and X always has 64 channels
WGRAD_TARGET_WORKGROUPS = 768       # sf_conv_wgrad_ex: about this many workgroups, 5 * CA / 64 per split
PARTIAL_SPLITS_MAX = 160            # sf_conv_wgrad_partial_floats(CA, 5) = 160 * CA * 1600


def scaled(tol, k):
    return (tol[0] * k, tol[1] * k)


def _both(v):
    return (v, v)


# What the tests assert.  Every form showed at least four times room against float64 at the project's bounds above on the MI355X, across all its cases,
# so each is tightened to about twice its measured worst (profiles/savi_train_kernel_tests.md holds both numbers per form); no bound goes below 2^-23, one
# float32 spacing of the largest reference element.  Keys: 'f32' / 'bf16x3' (the `precision` fixture: modes 0 / 1), 'bf16' (mode 2).
#   measured worst as a share of the project's bound:  wgrad f32 0.214, bf16x3 0.079, bf16 0.184;  dgrad f32 0.050, bf16x3 0.047, bf16 0.172;
#   conv0 f32 0.176, bf16x3 0.043, bf16 0.156;  head d_act f32 0.002, bf16x3 0.058, bf16 0.180;  head element-wise 0.020;  pos 0.003;
#   module (of 5 x the project's bound) f32 0.029, bf16x3 0.021
BOUNDS = {
    'wgrad': {'f32': _both(1e-5), 'bf16x3': _both(2e-5), 'bf16': _both(6e-3)},
    'dgrad': {'f32': _both(2.5e-6), 'bf16x3': _both(1.2e-5), 'bf16': _both(6e-3)},
    'first': {'f32': _both(1e-5), 'bf16x3': _both(1.2e-5), 'bf16': _both(6e-3)},
    'head_act': {'f32': _both(2**-23), 'bf16x3': _both(1.5e-5), 'bf16': _both(6e-3)},
    'head_f32': _both(1e-6),         # d_dec, d_out_w, d_out_b: float32 element-wise arithmetic and sums in every mode
    'pos': _both(2**-23),            # float32 sums in every mode
    # the module case: the project's per-launch bound times the number of chained contractions is 1e-4 (f32) / 5e-4 (bf16x3); first-order errors add,
    # but the errors of five launches do not line up, and the measured worst was 2.9e-6 / 1.05e-5
    'module': {'f32': _both(7e-6), 'bf16x3': _both(2.5e-5)},
}
PROJECT = {'f32': TOL['f32'], 'bf16x3': TOL['bf16x3'], 'bf16': TOL_BF16}


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient.  dW[n][k][ky][kx] = sum_(f,y,x) A[f,y,x,n] X[f, y s + ky - 2, x s + kx - 2, k];  A [F,H,W,CA], X [F,H s,W s,64]
# ---------------------------------------------------------------------------------------------------------------------
# name -> (F, H, W, s, CA, kernel form, splits, rps, empty splits)   with what the case reaches beside it
WGRAD_CASES = {
    # conv_wgrad_kernel: five shifted fetches, any grid
    'g_1x1': (1, 1, 1, 1, 64, 'generic', 1, 32, 0),          # one pixel: only the centre tap is non-zero
    'g_3x5': (2, 3, 5, 1, 64, 'generic', 1, 32, 0),          # 30 rows: one ragged chunk that straddles image rows and a frame
    'g_7x9': (3, 7, 9, 1, 64, 'generic', 3, 64, 0),          # 189 rows: 3 splits of 64, the last one 61 = 32 + 29
    'g_8x8_s2_ca128': (2, 8, 8, 2, 128, 'generic', 2, 64, 0),   # the decoder's first layer: two n tiles
    'g_16x16_s2': (3, 16, 16, 2, 64, 'generic', 12, 64, 0),  # 12 splits
    'g_4x6_s2': (2, 4, 6, 2, 64, 'generic', 1, 64, 0),       # off the square (48 rows in one split of 64)
    'g_4x4_s3': (1, 4, 4, 3, 64, 'generic', 1, 32, 0),       # a stride no reference decoder has
    # conv_wgrad_win_kernel<MODE, 1>: W % 32 == 0, one LDS window per 32-pixel chunk
    'w1_1x32': (1, 1, 32, 1, 64, 'win1', 1, 32, 0),          # Hx = 1: four of the five ky blocks are exactly zero
    'w1_64x64': (1, 64, 64, 1, 64, 'win1', 64, 64, 0),       # 64 splits of 64
    'w1_3x64x64': (3, 64, 64, 1, 64, 'win1', 153, 96, 25),   # rps 81 -> 96: the last 25 splits start past the last row
    'w1_10x32x32': (10, 32, 32, 1, 64, 'win1', 153, 96, 46),  # rps = 96 on 32-wide rows: a split holds three image rows
    'w1_2x128': (1, 2, 128, 1, 64, 'win1', 4, 64, 0),        # windows that start in the interior of a row (PHYRE's last layer)
    # conv_wgrad_win_kernel<MODE, 2>
    'w2_32x32': (2, 32, 32, 2, 64, 'win2', 32, 64, 0),
    'w2_32x32_ca128': (2, 32, 32, 2, 128, 'win2', 32, 64, 0),
    'w2_2x64': (1, 2, 64, 2, 64, 'win2', 2, 64, 0),          # 2 x 64 -> 4 x 128
}
WGRAD_NAMES = list(WGRAD_CASES)


def wgrad_plan(F_, H, W, s, CA):
    """(kernel form, splits, rows per split, empty trailing splits) of sf_conv_wgrad_ex, restated"""
    rows, nt = F_ * H * W, CA // 64
    splits = max(WGRAD_TARGET_WORKGROUPS // (KS * nt), 1)
    if splits * 64 > rows:
        splits = (rows + 63) // 64
    rps = -(-rows // splits)
    rps = (rps + 31) & ~31
    form = f'win{s}' if W % 32 == 0 and s in (1, 2) else 'generic'
    return form, splits, rps, splits - -(-rows // rps)


def wgrad_partial_floats(F_, H, W, s, CA):
    """floats of the partial buffer a call really needs: splits * CA * 1600"""
    return wgrad_plan(F_, H, W, s, CA)[1] * CA * KS * KS * CX


def _seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0xffff


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    """A [F,H,W,CA] ~ N(0, 1), X [F,Hs,Ws,64] ~ N(0.5, 1): with the non-zero mean of X a lost chunk is not hidden by cancellation"""
    F_, H, W, s, CA = WGRAD_CASES[name][:5]
    return rnd(F_, H, W, CA, seed=_seed(name)), rnd(F_, H * s, W * s, CX, seed=_seed(name) + 1) + 0.5


def wgrad_closed(a, x, s, mode='f64'):
    """the closed form: one [CA, rows] x [rows, 64] product per tap against the shifted, zero-padded X.  float64 [CA,64,5,5]"""
    F_, H, W, CA = a.shape
    xp = F.pad(x, (0, 0, 2, 2, 2, 2))
    out = torch.zeros(CA, CX, KS, KS, dtype=torch.float64)
    a2 = a.reshape(-1, CA)
    for ky in range(KS):
        for kx in range(KS):
            xs = xp[:, ky:ky + s * H:s, kx:kx + s * W:s, :].reshape(-1, CX)
            out[:, :, ky, kx] = product(lambda p, q: p.t() @ q, a2, xs, mode)
    return out


def wgrad_autograd(a, x, s):
    """float64 autograd of the transposed convolution whose input is A and whose output gradient is X (any s); at s = 1 this is also the weight
    gradient of the convolution whose input is X and whose output gradient is A (wgrad_autograd_conv): the same sum"""
    CA = a.shape[-1]
    w = torch.zeros(CA, CX, KS, KS, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(a.double().permute(0, 3, 1, 2), w, None, stride=s, padding=KS // 2, output_padding=s - 1)
    y.backward(x.double().permute(0, 3, 1, 2))
    return w.grad


def wgrad_autograd_conv(a, x):
    CA = a.shape[-1]
    w = torch.zeros(CA, CX, KS, KS, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, None, padding=KS // 2).backward(a.double().permute(0, 3, 1, 2))
    return w.grad


@functools.lru_cache(maxsize=None)
def wgrad_reference(name):
    a, x = wgrad_inputs(name)
    return wgrad_closed(a, x, WGRAD_CASES[name][3])


def wgrad_frame_reference(name, f):
    """the contribution of frame f alone"""
    a, x = wgrad_inputs(name)
    return wgrad_closed(a[f:f + 1], x[f:f + 1], WGRAD_CASES[name][3])


def onehot_pixels(H, W):
    """the four corners and one interior pixel of the A grid (fewer on degenerate grids); on rows wider than one 32-pixel chunk also the last pixel of
    the first chunk, whose X pixel two to the right is the last row of the window kernel's LDS window (tap kx = 4)"""
    out = []
    for p in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)) + (((H // 2, 31), ) if W > 32 else ()):
        if p not in out:
            out.append(p)
    return out


def onehot_case(name, i):
    """i-th one-hot run of a case: a single 1 in A at pixel i of onehot_pixels (channel n, frame f) and a single 1 in X (channel k, same frame) two
    pixels inwards of it along both axes, as far as the X grid goes.  Returns ((f, ya, xa, n), (f, yx, xx, k), (n, k, ky, kx)): the gradient is one
    exact 1 at [n][k][ky][kx] and exact zeros elsewhere."""
    F_, H, W, s, CA = WGRAD_CASES[name][:5]
    ya, xa = onehot_pixels(H, W)[i]
    f = (F_ - 1) if i % 2 == 0 else 0
    n, k = (CA - 1 - 37 * i) % CA, (5 + 13 * i) % CX
    Hx, Wx = H * s, W * s
    yx = min(max(ya * s + (2 if ya < H - 1 or H == 1 else -2), 0), Hx - 1)
    xx = min(max(xa * s + (2 if xa < W - 1 or W == 1 else -2), 0), Wx - 1)
    ky, kx = yx - ya * s + 2, xx - xa * s + 2
    assert 0 <= ky < KS and 0 <= kx < KS
    return (f, ya, xa, n), (f, yx, xx, k), (n, k, ky, kx)


def onehot_tensors(name, i):
    F_, H, W, s, CA = WGRAD_CASES[name][:5]
    pa, px, _ = onehot_case(name, i)
    a, x = torch.zeros(F_, H, W, CA), torch.zeros(F_, H * s, W * s, CX)
    a[pa] = 1.
    x[px] = 1.
    return a, x


def onehot_expected(name, i):
    CA = WGRAD_CASES[name][4]
    out = torch.zeros(CA, CX, KS, KS)
    out[onehot_case(name, i)[2]] = 1.
    return out


# ---------------------------------------------------------------------------------------------------------------------
# masked data gradient.  out = mask > 0 ? Conv2d(5, stride, padding 2)(g) : 0;  g [F,Hin,Win,Cin], w_packed [Cout][5][5][Cin], out and mask
# [F,Hin/s,Win/s,Cout].  `route`: how the weight reaches the kernel and which autograd the reference is --
#   'conv'   : a Conv2d weight [Cin_g, Cout_o, 5, 5] (its c_out is the gradient's channel count) through sf_pack_conv_bwd_weight_f32; the reference is
#              the input gradient of F.conv2d (the encoder's layers), stride 1
#   'deconv' : a ConvTranspose2d weight [Cout_o, Cin_g, 5, 5] through sf_pack_conv_weight_f32; the reference is the input gradient of
#              F.conv_transpose2d (the decoder's layers), any stride
# ---------------------------------------------------------------------------------------------------------------------
# name -> (F, Hin, Win, stride, Cin (of the gradient), Cout, route, masked)
DGRAD_CASES = {}
for _F in (1, 3):
    for _H in (2, 4, 6, 8):      # W = 64: rows4 (H % 4 == 0, split-bf16, fragment weights), halo (H % 2 == 0 or mode 2), GEMM epilogue (f32 mode)
        DGRAD_CASES[f's1_w64_f{_F}_h{_H}'] = (_F, _H, 64, 1, 64, 64, 'conv', True)
DGRAD_CASES.update({
    's1_8x8': (2, 8, 8, 1, 64, 64, 'conv', True),             # off-shape: the GEMM epilogue in every mode
    's1_5x7': (1, 5, 7, 1, 64, 64, 'conv', True),             # odd sizes, M = 35: one ragged tile
    's1_8x8_co128': (2, 8, 8, 1, 64, 128, 'deconv', True),    # 64 -> 128: the adjoint of the decoder's first layer at stride 1, two column tiles
    's2_4x4': (2, 4, 4, 2, 64, 64, 'deconv', True),           # -> 2 x 2
    's2_4x4_nomask': (2, 4, 4, 2, 64, 64, 'deconv', False),
    's2_16x16': (3, 16, 16, 2, 64, 64, 'deconv', True),       # -> 8 x 8: 192 rows, two row tiles
    's2_16x16_nomask': (3, 16, 16, 2, 64, 64, 'deconv', False),
    's2_6x4': (1, 6, 4, 2, 64, 64, 'deconv', True),           # -> 3 x 2: off the square
    's2_6x4_nomask': (1, 6, 4, 2, 64, 64, 'deconv', False),
})
DGRAD_NAMES = list(DGRAD_CASES)


def mask_pattern(shape, seed):
    """a ReLU mask as an input: +1, -1, +0.0, -0.0 and normal values in equal shares, another pattern in every frame"""
    rs = np.random.RandomState(seed)
    kind = rs.randint(0, 5, size=shape)
    vals = rs.standard_normal(shape).astype(np.float32)
    out = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [np.float32(1), np.float32(-1), np.float32(0.), np.float32(-0.)], vals)
    return torch.from_numpy(out.astype(np.float32))


@functools.lru_cache(maxsize=None)
def dgrad_inputs(name):
    """(g [F,Hin,Win,Cin], torch-layout weight, mask [F,Ho,Wo,Cout] or None)"""
    F_, Hin, Win, s, Cin, Cout, route, masked = DGRAD_CASES[name]
    sd = _seed(name)
    g = rnd(F_, Hin, Win, Cin, seed=sd)
    wshape = (Cin, Cout, KS, KS) if route == 'conv' else (Cout, Cin, KS, KS)
    w = rnd(*wshape, seed=sd + 1, scale=(KS * KS * Cin)**-0.5)
    mask = mask_pattern((F_, Hin // s, Win // s, Cout), sd + 2) if masked else None
    return g, w, mask


def dgrad_packed(w, route):
    """what sf_pack_conv_bwd_weight_f32 ('conv') / sf_pack_conv_weight_f32 ('deconv') make of the torch weight: [Cout][ky][kx][Cin]"""
    if route == 'conv':      # w [co_fwd = Cin_g, ci_fwd = Cout_o, ky, kx] -> [ci_fwd][4 - ky][4 - kx][co_fwd]
        return w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    return w.permute(0, 2, 3, 1).contiguous()


def dgrad_closed(g, w_packed, s, mask, mode='f64'):
    F_, Hin, Win, Cin = g.shape
    Cout = w_packed.shape[0]
    Ho, Wo = Hin // s, Win // s
    gp = F.pad(g, (0, 0, 2, 2, 2, 2))
    out = torch.zeros(F_ * Ho * Wo, Cout, dtype=torch.float64)
    for ky in range(KS):
        for kx in range(KS):
            gs = gp[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s, :].reshape(-1, Cin)
            out += product(lambda p, q: p @ q.t(), gs, w_packed[:, ky, kx, :], mode)
    out = out.view(F_, Ho, Wo, Cout)
    return out if mask is None else torch.where(mask > 0, out, torch.zeros_like(out))


def dgrad_autograd(g, w, s, route, mask):
    F_, Hin, Win, Cin = g.shape
    g64 = g.double().permute(0, 3, 1, 2)
    if route == 'conv':
        x = torch.zeros(F_, w.shape[1], Hin, Win, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w.double(), None, padding=KS // 2).backward(g64)
    else:
        x = torch.zeros(F_, w.shape[0], Hin // s, Win // s, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, w.double(), None, stride=s, padding=KS // 2, output_padding=s - 1).backward(g64)
    out = x.grad.permute(0, 2, 3, 1).contiguous()
    return out if mask is None else torch.where(mask > 0, out, torch.zeros_like(out))


@functools.lru_cache(maxsize=None)
def dgrad_reference(name):
    g, w, mask = dgrad_inputs(name)
    s, route = DGRAD_CASES[name][3], DGRAD_CASES[name][6]
    return dgrad_closed(g, dgrad_packed(w, route), s, mask)


def dgrad_form(name, precision):
    """which implementation sf_conv2d_nhwc_bwd_data_f32 takes ('halo' / 'gemm'); 'rows4' is reached through sf_conv5x5_frag_f32 (and by the module
    paths) where dgrad_rows4(name) holds, in split-bf16 mode only"""
    F_, Hin, Win, s, Cin, Cout, _, _ = DGRAD_CASES[name]
    if s == 1 and Win == 64 and Cin == 64 and Cout == 64 and Hin % 2 == 0 and precision in ('bf16x3', 'bf16'):
        return 'halo'
    return 'gemm'


def dgrad_rows4(name):
    F_, Hin, Win, s, Cin, Cout, _, masked = DGRAD_CASES[name]
    return s == 1 and Win == 64 and Cin == 64 and Cout == 64 and Hin % 4 == 0


# ---------------------------------------------------------------------------------------------------------------------
# conv0's weight gradient against the image patches
# ---------------------------------------------------------------------------------------------------------------------
FIRST_CASES = {'r64': (1, 64, 0), 'r128_gap': (2, 128, 1000)}     # name -> (F, resolution, floats between two frames: NaN-filled)


@functools.lru_cache(maxsize=None)
def first_inputs(name):
    F_, res, _ = FIRST_CASES[name]
    return rnd(F_, 3, res, res, seed=_seed(name)) + 0.25, rnd(F_ * 4096, 64, seed=_seed(name) + 1)


def first_closed(img, dy, mode='f64'):
    res = img.shape[-1]
    P = F.unfold(img, KS, padding=KS // 2, stride=res // 64)                    # [F, 75, 4096], k = (ci, ky, kx): the torch weight order
    P = P.permute(0, 2, 1).reshape(-1, 3 * KS * KS)
    return product(lambda p, q: p.t() @ q, dy, P, mode).view(64, 3, KS, KS)


def first_autograd(img, dy):
    res, F_ = img.shape[-1], img.shape[0]
    w = torch.zeros(64, 3, KS, KS, dtype=torch.float64, requires_grad=True)
    F.conv2d(img.double(), w, None, stride=res // 64, padding=KS // 2).backward(dy.double().view(F_, 64, 64, 64).permute(0, 3, 1, 2))
    return w.grad


# ---------------------------------------------------------------------------------------------------------------------
# position-embedding gradients and the decoder's head block (float32 element-wise kernels; the head's masked K = 4 product is a GEMM)
# ---------------------------------------------------------------------------------------------------------------------
POS_CASES = [(1, 1, 64), (3, 4, 128), (5, 300, 64), (2, 4096, 64), (2, 16, 4)]      # (F, HW, C)


@functools.lru_cache(maxsize=None)
def pos_inputs(F_, HW, C_):
    return rnd(F_, HW, C_, seed=F_ + HW + C_) + 0.3, torch.from_numpy(np.random.RandomState(HW).rand(HW, 4).astype(np.float32))


def pos_reference(d, grid):
    tab = d.double().sum(0)
    return tab.t() @ grid.double(), tab.sum(0), tab


def pos_autograd(d, grid):
    C_ = d.shape[-1]
    w = torch.zeros(C_, 4, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C_, dtype=torch.float64, requires_grad=True)
    ((F.linear(grid.double(), w, b).unsqueeze(0) + torch.zeros_like(d, dtype=torch.float64)) * d.double()).sum().backward()
    return w.grad, b.grad


# name -> (F, N, HW, Cl, gain on the mask logits)
HEAD_CASES = {
    'n1': (1, 1, 16, 64, 1.),            # N = 1: the mask-logit gradient is exactly zero
    'n3': (2, 3, 64, 64, 1.),
    'n3_rows2304': (3, 3, 256, 64, 1.),  # 2304 rows: rpg = 5, the four row lanes of head_grad_partial_kernel really stride
    'cl8': (1, 16, 1024, 8, 1.),         # Cl < 64
    'saturated': (2, 3, 64, 64, 64.),    # the mask logits times decode_cases.MASK_GAIN: the softmax saturates
}
HEAD_NAMES = list(HEAD_CASES)


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """dec [F,N,HW,4], d_recon [F,3,HW], act [F*N*HW,Cl] (a mask pattern: only its sign gates, its values enter d_out_w), out_w [4,Cl]"""
    F_, N, HW, Cl, gain = HEAD_CASES[name]
    sd = _seed(name)
    dec = rnd(F_, N, HW, 4, seed=sd)
    dec[..., 3] *= gain
    return dec, rnd(F_, 3, HW, seed=sd + 1), mask_pattern((F_ * N * HW, Cl), sd + 2), rnd(4, Cl, seed=sd + 3, scale=Cl**-0.5)


def head_d_dec_closed(dec, d_recon):
    dec, g = dec.double(), d_recon.double().permute(0, 2, 1).unsqueeze(1)      # g [F,1,HW,3]
    m = torch.softmax(dec[..., 3:], dim=1)
    rg = (dec[..., :3] * g).sum(-1, keepdim=True)
    return torch.cat([m * g, m * (rg - (m * rg).sum(1, keepdim=True))], -1)


def head_d_dec_autograd(dec, d_recon):
    d = dec.double().requires_grad_(True)
    recon = (d[..., :3] * torch.softmax(d[..., 3:], dim=1)).sum(1)             # [F,HW,3]
    recon.backward(d_recon.double().permute(0, 2, 1))
    return d.grad


def head_d_act(d_dec, act, out_w, mode='f64'):
    y = product(lambda p, q: p @ q, d_dec.reshape(-1, 4).float(), out_w, mode)
    return torch.where(act > 0, y, torch.zeros_like(y))


def head_param_grads(d_dec, act):
    d = d_dec.reshape(-1, 4).double()
    return d.t() @ act.double(), d.sum(0)


def head_rpg(F_, N, HW):
    rows = F_ * N * HW
    return -(-rows // 512)


# ---------------------------------------------------------------------------------------------------------------------
# module wiring: decode_cases.TRAIN_CASE through StoSAVi.decode under autograd.  No ReLU of its float64 forward is within decode_cases.KINK_MARGIN of
# its kink (tests/test_savi_train_kernel_cases.py), ten times the forward error measured for these convolutions (profiles/decode_tests.md), so the
# device's forward takes the reference's branches and the gradients compare element by element.  The bound: the per-launch bound times the number of
# chained contractions on the path -- dec_layers transposed convolutions, the head, and the weight gradient or adjoint that ends it; first-order
# errors add.
# ---------------------------------------------------------------------------------------------------------------------
MODULE_RECON_BOUND = 2e-4        # max |err| / max |ref| of the forward: tests/test_decode_gpu.py


def module_chain():
    import decode_cases as dc
    return len(dc.TRAIN_CASES[dc.TRAIN_CASE][3]) - 1 + 2


def module_param_names():
    import decode_cases as dc
    L = len(dc.TRAIN_CASES[dc.TRAIN_CASE][3]) - 1
    return ([f'decoder.{i}.0.{p}' for i in range(L) for p in ('weight', 'bias')] + [f'decoder.{L}.weight', f'decoder.{L}.bias'] +
            ['decoder_pos_embedding.dense.weight', 'decoder_pos_embedding.dense.bias'])


@functools.lru_cache(maxsize=None)
def module_d_recon():
    import decode_cases as dc
    res, _, _, _, _, _, F_ = dc.TRAIN_CASES[dc.TRAIN_CASE]
    return rnd(F_, 3, res, res, seed=77)


@functools.lru_cache(maxsize=None)
def module_reference():
    """float64 autograd of oracle.savi_decode on decode_cases.train_case(): dict(recon, d_slots, grads {parameter name: gradient})"""
    import decode_cases as dc
    import oracle
    _, sd64, cfg, slots = dc.train_case()
    names = module_param_names()
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd64.items()}
    so = slots.double().requires_grad_(True)
    recon = oracle.savi_decode(so, osd, cfg)[0]
    recon.backward(module_d_recon().double())
    return dict(recon=recon.detach(), d_slots=so.grad, grads={k: osd[k].grad for k in names})
