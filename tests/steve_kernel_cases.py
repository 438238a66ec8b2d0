"""Case tables and float64 references of the STEVE token-side forward kernels (csrc/steve_decoder.hip), shared by
tests/test_steve_kernel_cases.py (CPU) and tests/test_steve_kernels_gpu.py.  Plain torch on the CPU; the library is not imported here.

Every reference is computed in float64 from the float32 inputs the kernel gets, once per case (lru_cache): do not write into one.
Every case is the smallest shape that still takes the branch named beside it; the branch conditions are those of
sf_slate_attention_strided_f32, softmax_rows_launch, sf_softmax_rows_bwd_f32 and the kernels' own loops.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# |a - b| <= rtol |b| + floor max|b|, element by element (tests/test_train_kernels_gpu.close)
TOL = {'f32': (2e-5, 2e-5), 'bf16x3': (1e-4, 1e-4)}   # matrix products, per precision mode
TOL_ATTN_F32 = (2e-5, 2e-5)                           # slate_attn_kernel / slate_decode_attn_kernel: plain float32 in every mode
# row kernels: the project's rtol; floor 1e-6 = 8 ulp of the largest output (the absolute term of the cross-entropy bound).  The inputs
# of the ordinary table are 0.4 N(0, 1), so that |z| <= 30 at scale 10 and the roundings of (x + add) * scale, two of 2^-24 |z| on
# the element and on the row maximum, stay below 2 * 30 * 1.2e-7 = 7.2e-6 relative to exp(c): inside rtol without help from the floor.
TOL_ROWS = (1e-5, 1e-6)
TOL_GN = (1e-5, 1e-5)
HEAD_DIMS = (16, 32, 48, 64)


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def err_over_bound(a, b, tol, keep=None, per_row=False):
    """largest |a - b| / (rtol |b| + floor max|b|) over the elements (of the boolean mask `keep`); per_row: max|b| of the element's
    own row instead of the whole tensor's, the stricter form for rows of very different size"""
    rtol, floor = tol
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    bound = (rtol * b.abs() + floor * (b.abs().max(-1, keepdim=True)[0] if per_row else b.abs().max())).clamp_min(1e-300)
    ratio = (a - b).abs() / bound
    if keep is not None:
        ratio = ratio[keep]
    return ratio.max().item() if ratio.numel() else 0.


# ---------------------------------------------------------------------------------------------------------------------
# slate attention.  Dispatch of sf_slate_attention_strided_f32:
#   causal and Lq >= 128      -> slate_flash_bf3_kernel<hd> (precision mode >= 1) or slate_flash_kernel<hd> (mode 0), 64-query tiles
#   Lq == 1 and not causal    -> slate_decode_attn_kernel<hd>, the keys spread over 256 threads
#   everything else           -> slate_attn_kernel<hd>, 256 queries per workgroup, keys in tiles of 64
# ---------------------------------------------------------------------------------------------------------------------
FLASH_L = {
    128: 'threshold: two full tiles, no ragged row',
    129: 'last query tile with one live row',
    191: 'one full tile, ragged diagonal tile (63 rows); key tile 1 of query tile 2 is not `full` (k0 + 64 > L)',
    192: 'three full tiles: the `full` shortcut on every tile below the diagonal',
    193: 'full tiles followed by a one-row diagonal tile',
    257: 'four full tiles and a one-row fifth',
}
FLASH_CASES = [(L, hd) for L in FLASH_L for hd in HEAD_DIMS]

GENERIC_CAUSAL_L = {
    1: 'one query, one key (causal, so not the decode kernel)',
    2: 'two rows',
    63: 'ragged single key tile',
    64: 'exactly one key tile',
    65: 'second key tile with one key',
    127: 'the last length below the flash threshold',
}
GENERIC_CAUSAL_CASES = [(L, hd) for L in GENERIC_CAUSAL_L for hd in HEAD_DIMS]

# (Lq, Lk, hd): every head dim occurs
GENERIC_CROSS_CASES = [
    (2, 1, 16),       # one key; Lq = 2 keeps it off the decode kernel
    (70, 6, 32),      # the slot cross-attention shape
    (64, 7, 48),
    (65, 64, 64),     # exactly one key tile
    (130, 65, 16),    # second key tile with one key
    (255, 11, 32),    # one dead thread
    (256, 16, 48),    # a full workgroup
    (257, 130, 64),   # a second workgroup in x with one live query, three key tiles
    (300, 6, 16),     # Lq > 256
]

DECODE_LK = {
    1: 'one key: 255 threads and three waves own none',
    2: 'two keys',
    63: 'waves 1-3 own no key',
    64: 'wave 0 full, waves 1-3 empty',
    65: 'wave 1 owns one key',
    255: 'one thread without a key',
    256: 'one key per thread',
    257: 'thread 0 gets its second key',
    513: 'thread 0 gets its third key',
    1025: 'max_len + 1 of the 128 x 128 model',
}
DECODE_CASES = [(Lk, hd) for Lk in DECODE_LK for hd in HEAD_DIMS]
CACHE_SPARE_ROWS = 7

TRAIN_FWD_L = {127: 'slate_attn_fwd_train_kernel (the short form)', 128: 'flash, TRAIN', 129: 'flash, TRAIN, one-row tile',
               193: 'flash, TRAIN, full tile + ragged diagonal'}
TRAIN_FWD_CASES = [(L, hd) for L in TRAIN_FWD_L for hd in HEAD_DIMS]


@functools.lru_cache(maxsize=None)
def attention_case(B, H, hd, Lq, Lk, causal, seed=0):
    """dict(q, k, v float32 [B,L,d]; out float64 [B,Lq,d]; lse float64 [B,H,Lq]; smax = max |score| over the unmasked pairs)"""
    d = H * hd
    q, k, v = rnd(B, Lq, d, seed=seed + 1), rnd(B, Lk, d, seed=seed + 2), rnd(B, Lk, d, seed=seed + 3)
    out, lse, smax = attention_ref(q, k, v, H, causal)
    return dict(q=q, k=k, v=v, out=out, lse=lse, smax=smax)


def attention_ref(q, k, v, H, causal):
    B, Lq, d = q.shape
    Lk, hd = k.shape[1], d // H
    qh, kh, vh = (t.double().view(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * hd**-0.5
    smax = s.abs().max().item()
    if causal:
        assert Lq == Lk
        dead = torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)
        smax = s.masked_fill(dead, 0.).abs().max().item()
        s = s.masked_fill(dead, float('-inf'))
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, d)
    return out, torch.logsumexp(s, -1), smax


# ---------------------------------------------------------------------------------------------------------------------
# row kernels.  softmax_rows_launch / sf_softmax_rows_bwd_f32: reg<1> if V % 4 == 0, V <= 1024 and all pointers 16-byte aligned;
# reg<4> if V % 4 == 0 and V <= 4096 and aligned; the generic kernel otherwise.
# ---------------------------------------------------------------------------------------------------------------------
ROWS_R = 5
ROW_V = {
    1: 'generic (V % 4 != 0): one element, 255 idle threads',
    4: 'reg<1>: one float4, one live thread',
    64: 'reg<1>: 16 live threads of wave 0',
    255: 'generic: one idle thread',
    1020: 'reg<1>: thread 255 idle',
    1024: 'reg<1>: its last size',
    1028: 'reg<4>: its first size, one float4 in the second pass',
    4092: 'reg<4>: ragged fourth pass',
    4096: 'reg<4>: its last size',
    4100: 'generic: the first size past reg<4> with V % 4 == 0',
    5000: 'generic: 20 strided passes, ragged',
}
SOFTMAX_FORMS = [(False, 1.0), (False, 10.0), (True, 1.0), (True, 10.0)]   # (add, scale)
LARGE_LOGIT_V = {1024: 'reg<1>', 4096: 'reg<4>', 5000: 'generic'}
LARGE_LOGIT_SCALE = 10.0


def softmax_ref(x, add, scale, log=False):
    z = (x.double() + (add.double() if add is not None else 0.)) * scale
    return torch.log_softmax(z, -1) if log else torch.softmax(z, -1)


@functools.lru_cache(maxsize=None)
def softmax_case(V, with_add, scale, log=False):
    x = rnd(ROWS_R, V, seed=V + 11, scale=0.4)
    add = rnd(ROWS_R, V, seed=V + 12, scale=0.4) if with_add else None
    return dict(x=x, add=add, ref=softmax_ref(x, add, scale, log))


@functools.lru_cache(maxsize=None)
def softmax_bwd_case(V, scale):
    """y = a float32 softmax output, dy ~ N(0, 1); ref = scale * y * (dy - sum(y dy)) in float64.  y is the softmax of N(0, 1) logits
    at either scale: next to a one-hot y the factor dy - sum(y dy) of the dominant entry cancels to the size of the rest of the row, and
    the rounding of the float32 dot product, harmless to every other entry, would be all that is left of it."""
    y = softmax_ref(rnd(ROWS_R, V, seed=V + 13), None, 1.0).float()
    dy = rnd(ROWS_R, V, seed=V + 14)
    y64, g64 = y.double(), dy.double()
    return dict(y=y, dy=dy, ref=scale * y64 * (g64 - (y64 * g64).sum(-1, keepdim=True)))


@functools.lru_cache(maxsize=None)
def large_logit_case(V):
    """rows with max |z| = 300 after scaling: row 0 one dominant entry over non-positive ones, rows 1-2 normal logits stretched to
    |x| <= 30, rows 3-4 a crowd within a few units of its maximum at +300 / at -290 (where the rounding of z = (x + add) * scale, 2^-24 |z| twice,
    reaches exp(c) undamped).  x_log = the same logits for sf_log_softmax_rows_f32 (no scale there)."""
    x = rnd(ROWS_R, V, seed=V + 21)
    x = x / x.abs().max(-1, keepdim=True)[0] * 30.
    x[0] = -x[0].abs()
    x[0, 7 % V] = 30.
    crowd = 30. - 0.3 * rnd(2, V, seed=V + 22).abs()
    x[3], x[4] = crowd[0], crowd[1] - 59.
    add = rnd(ROWS_R, V, seed=V + 23, scale=0.1)
    x_log = ((x + add) * LARGE_LOGIT_SCALE).contiguous()
    return dict(x=x, add=add, scale=LARGE_LOGIT_SCALE, x_log=x_log, ref=softmax_ref(x, add, LARGE_LOGIT_SCALE),
                ref_log=softmax_ref(x_log, None, 1.0, log=True), t32=torch.softmax((x + add) * LARGE_LOGIT_SCALE, -1),
                t32_log=torch.log_softmax(x_log, -1), zmax=((x.double() + add.double()) * LARGE_LOGIT_SCALE).abs().max(-1)[0])


# cross-entropy: xent_rows_kernel (one workgroup per row, strided passes) + mean_kernel (double accumulation)
XENT_V = (1, 64, 255, 1000, 4096, 4097, 10000)
XENT_R = (1, 37)
XENT_CASES = [(V, R) for V in XENT_V for R in XENT_R]
XENT_RTOL, XENT_ATOL, XENT_MEAN_RTOL = 1e-5, 1e-6, 1e-6


@functools.lru_cache(maxsize=None)
def xent_case(V, R):
    """logits 3 N(0, 1).  R = 1: target V - 1.  R = 37: row 0 target 0, row 1 target V - 1, row 2 target = its maximum, row 3 (V > 1)
    target logit exactly 200 below the maximum, the rest seeded."""
    x = rnd(R, V, seed=V + R, scale=3.0)
    tgt = torch.from_numpy(np.random.RandomState(V + R + 1).randint(0, V, size=R)).long()
    if R == 1:
        tgt[0] = V - 1
    else:
        tgt[0], tgt[1] = 0, V - 1
        tgt[2] = x[2].argmax()
        if V > 1:
            tgt[3] = (int(x[3].argmax()) + 1) % V
            x[3, tgt[3]] = x[3].max() - 200.
    rows = -torch.log_softmax(x.double(), -1).gather(1, tgt[:, None])[:, 0]
    return dict(x=x, tgt=tgt, rows=rows, mean=rows.mean())


# arg-max: thread t owns the indices t, t + 256, ...; lanes merge inside a wave (index < 64 -> wave 0, ... < 256 -> wave 3), then the
# four waves.  Rows that hold a NaN are unspecified and not tested.
ARGMAX_V = (1, 63, 64, 255, 256, 257, 4096, 5000)
ARGMAX_LD_EXTRA = 3
TIE_VALUE = 10.0   # above every 1 N(0, 1) entry of the rows
NEG_INF = float('-inf')


def argmax_rows_table(V):
    """list of (what, ties, expected): `ties` = the indices set to TIE_VALUE (None: an all -inf row), expected = the first of them"""
    rows = [('maximum at index 0', (0, ), 0), ('maximum at index V - 1', (V - 1, ), V - 1)]
    if V > 1:
        rows.append(('ties at 0 and V - 1', (0, V - 1), 0))
    if V >= 41:
        rows.append(('two lanes of wave 0', (3, 40), 3))
    if V >= 131:
        rows += [('two waves', (10, 100), 10), ('two waves, the later index in the lower lane', (100, 130), 100)]
    if V >= 257:
        rows.append(('one thread, indices j and j + 256', (V - 257, V - 1), V - 257))
    if V >= 262:
        rows += [('one thread, indices 5 and 261', (5, 261), 5), ('thread 200 before the second element of thread 5', (200, 261), 200)]
    rows += [('all -inf', None, 0), ('-inf after masking', None, 0)]
    return rows


@functools.lru_cache(maxsize=None)
def argmax_case(V):
    """dict(x float32 [R, V], expected int64 [R], table).  The last row but one is filled with -inf, the last one is seeded logits plus
    a mask of -inf on every column; one more row keeps a single finite entry at V - 1 behind -inf everywhere else."""
    table = argmax_rows_table(V)
    x = rnd(len(table) + 1, V, seed=V + 31)
    for r, (_, ties, _) in enumerate(table):
        if ties is None:
            x[r] = x[r] + NEG_INF if r == len(table) - 1 else NEG_INF
        else:
            x[r, list(ties)] = TIE_VALUE
    x[-1, :V - 1] = NEG_INF
    expected = torch.tensor([e for _, _, e in table] + [V - 1 if V > 1 and x[-1, V - 1] > NEG_INF else 0])
    return dict(x=x, expected=expected, table=table)


# token embedding: embed_kernel, one thread per float4; (B, L, d, vocabulary rows)
EMBED_CASES = [
    (3, 5, 4, 9),       # 15 float4: one partly filled workgroup
    (2, 41, 64, 50),    # 1312 float4: six workgroups, the last one ragged
    (3, 7, 192, 33),    # 1008 float4
]


@functools.lru_cache(maxsize=None)
def embed_case(B, L, d, rows):
    """pos has exactly L rows; the last table row and row 0 occur as tokens"""
    emb, pos = rnd(rows, d, seed=d + 41), rnd(L, d, seed=d + 42)
    idx = torch.from_numpy(np.random.RandomState(d + 43).randint(0, rows, size=(B, L))).long()
    idx[0, 0], idx[-1, -1] = rows - 1, 0
    return dict(emb=emb, pos=pos, idx=idx, ref=emb[idx] + pos[None])


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm(1 group) (+ ReLU, + PixelShuffle(2)) on NHWC: gn_stats_kernel reduces n / 4 float4 of a sample in GN_P = 64 slices
# ---------------------------------------------------------------------------------------------------------------------
GN_P = 64
GN_SHAPES = {   # (F, H, W, C, shuffle)
    (1, 1, 1, 4, 1): 'n / 4 = 1: 63 empty slices',
    (2, 1, 3, 16, 1): 'n / 4 = 12: 52 empty slices',
    (3, 4, 6, 64, 2): 'H != W with pixel shuffle; n / 4 = 384, 6 float4 per slice',
    (2, 8, 16, 64, 1): 'n / 4 = 2048: 32 per slice, threads 32-255 idle',
    (1, 32, 32, 64, 1): 'n / 4 = 16384 = GN_P * 256: every thread one float4',
    (2, 5, 7, 48, 1): 'n / 4 = 420, per = 7: does not divide, slices 60-63 empty',
}
GN_CASES = [s + (relu, ) for s in GN_SHAPES for relu in (True, False)]
GN_KINK = 1e-6
GN_COND_SHAPE = (1, 32, 32, 64)
GN_COND_RATIOS = (0.25, 8.)      # asserted at TOL_GN
GN_COND_LIMIT = 32.              # measured only: var = E[x^2] - mean^2 over float block sums


def groupnorm_ref(x, g, b, relu, shuffle, eps=1e-5):
    """x NHWC float32 -> (float64 NHWC output, boolean mask of the elements excluded at the ReLU kink)"""
    pre = F.group_norm(x.double().permute(0, 3, 1, 2), 1, g.double(), b.double(), eps)
    y = torch.relu(pre) if relu else pre          # the branch is the float64 reference's own sign
    excluded = (pre.abs() < GN_KINK) if relu else torch.zeros_like(pre, dtype=torch.bool)
    if shuffle == 2:
        y, excluded = F.pixel_shuffle(y, 2), F.pixel_shuffle(excluded.double(), 2) > 0
    return y.permute(0, 2, 3, 1).contiguous(), excluded.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def groupnorm_case(F_, H, W, C, shuffle, relu, ratio=None):
    """ratio None: x = 0.5 + 2 N(0, 1) as in test_kernels_gpu; otherwise x = ratio + N(0, 1) (mean / std = ratio)"""
    x = rnd(F_, H, W, C, seed=C + H, scale=2.0) + 0.5 if ratio is None else rnd(F_, H, W, C, seed=C + H) + ratio
    g, b = 1 + 0.1 * rnd(C, seed=C + 51), 0.1 * rnd(C, seed=C + 52)
    ref, excluded = groupnorm_ref(x, g, b, relu, shuffle)
    return dict(x=x, g=g, b=b, ref=ref, excluded=excluded)
