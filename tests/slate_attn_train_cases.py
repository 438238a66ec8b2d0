"""Case table and float64 reference of STEVE's training attention (csrc/slate_attn_bwd.hip and the TRAIN instantiation of the flash
kernels in csrc/steve_decoder.hip), shared by tests/test_slate_attn_train_cases.py (CPU) and tests/test_slate_attn_train_gpu.py.
Plain torch / numpy on the CPU; no library call (slotformer_amd.train.dropout_keep_mask is the host restatement of the mask).

The reference is computed twice in float64 from the float32 inputs the kernels get, once per case (lru_cache): by autograd, and from the
closed form the kernels implement.  The CPU test holds the two to 1e-12 of each other: do not write into either.
Every case is the smallest shape that reaches the edge named beside it: B <= 3, H <= 3, no length above 257, but for the one case at the
workload's own head.  The table is a covering design, not a cross product: see the rules above CASES.
"""
import collections
import functools

import numpy as np
import torch

import steve_kernel_cases as sc
from steve_kernel_cases import attention_case, err_over_bound, rnd   # noqa: F401  (re-exported for the two test files)

SEED = 0x5eed00001234
MODES = ('f32', 'bf16x3')

# |a - b| <= rtol |b| + floor max|b|, element by element, per kernel and precision mode.  The starting point is what the project
# promises for matrix products, steve_kernel_cases.TOL = (2e-5, 2e-5) in exact f32 and (1e-4, 1e-4) in split-bf16.  Wherever the worst
# error measured against float64 over every call of the GPU tests left more than a factor of 4 of that, the bound is twice the worst
# measured error, rounded up to one digit (twice: dq's atomics make its last bits vary from run to run); profiles/slate_attn_train.md
# holds the measurements.  lse is held to rtol max|score| + floor with the same pair.
def _both(x):
    return (x, x)


TOL_FWD = {
    ('fwd_train<32>', 'f32'): _both(6e-7), ('fwd_train<64>', 'f32'): _both(2e-6), ('flash<TRAIN>', 'f32'): _both(4e-7),
    ('fwd_train<32>', 'bf16x3'): _both(3e-5), ('fwd_train<64>', 'bf16x3'): _both(3e-5), ('flash_bf3<TRAIN>', 'bf16x3'): _both(2e-5),
}
TOL_BWD = {
    ('bwd<32>', 'f32'): _both(2e-6), ('bwd<64>', 'f32'): _both(2e-6),
    ('bwd<32>', 'bf16x3'): sc.TOL['bf16x3'],      # worst measured 0.30 of it: stays
    ('bwd48v2', 'bf16x3'): sc.TOL['bf16x3'],      # worst measured 0.33 of it: stays
    ('bwd<64>', 'bf16x3'): _both(4e-5),
}
# the max-norm figures of tests/test_kernels_gpu.py::test_slate_attention_backward, asserted next to the element-wise bound so that
# nothing here is looser than what the same kernel is held to there
MAXNORM_BWD = {'f32': 2e-5, 'bf16x3': 2e-4}


# ---------------------------------------------------------------------------------------------------------------------
# which kernel a call takes, restated from the entry points
# ---------------------------------------------------------------------------------------------------------------------
def bwd_kernel_of(hd, mode, ldk, ldv, kv_aligned=True):
    """sf_slate_attention_train_bwd_f32.  kv_aligned: k, v and their batch strides are multiples of 16 bytes.  None: refused."""
    if not (4 <= hd <= 64 and hd % 4 == 0):        # SF_REQUIRE(head_dim >= 4 && head_dim <= 64 && head_dim % 4 == 0, ...)
        return None
    kv16 = ldk % 4 == 0 and ldv % 4 == 0 and kv_aligned   # const bool kv16 = ldk % 4 == 0 && ldv % 4 == 0 && k_bs % 4 == 0 && ...
    if mode == 'bf16x3' and 32 < hd <= 48 and kv16:       # if (bf3 && head_dim > 32 && head_dim <= 48 && bwd48 && kv16)
        return 'bwd48v2'
    return 'bwd<32>' if hd <= 32 else 'bwd<64>'    # const int hdp = head_dim <= 32 ? 32 : 64;


def fwd_kernel_of(hd, L, causal, mode):
    """sf_slate_attention_train_fwd_f32; L = Lq.  None: refused."""
    if not (2 <= hd <= 64 and hd % 2 == 0):        # SF_REQUIRE(head_dim >= 2 && head_dim <= 64 && head_dim % 2 == 0, ...)
        return None
    if causal and L >= 128 and hd in (16, 32, 48, 64):   # sf_slate_flash_train_ex: if (L < 128 || !(head_dim == 16 || ... == 64)) return 1;
        return 'flash_bf3<TRAIN>' if mode == 'bf16x3' else 'flash<TRAIN>'   # if (head_dim == HD_ && sf_get_precision() >= 1 && ...)
    return 'fwd_train<32>' if hd <= 32 else 'fwd_train<64>'   # const int hdp = head_dim <= 32 ? 32 : 64;


def is_full(L_q, L_k, causal, qb, kb):
    """the 48-wide kernel's shortcut: (!p.causal || qb > kb) && q0 + 64 <= p.Lq && k0 + 64 <= p.Lk"""
    return (not causal or qb > kb) and qb * 64 + 64 <= L_q and kb * 64 + 64 <= L_k


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'B H hd Lq Lk causal p bwd edge')

HD_W32, HD_W48, HD_W64, HD_FWD_ONLY = (4, 12, 16, 28, 32), (36, 40, 44, 48), (52, 60, 64), (2, 18, 50)
BWD_HEAD_DIMS = HD_W32 + HD_W48 + HD_W64
CAUSAL_L = {
    1: 'Lq = Lk = 1',
    2: 'two rows',
    63: 'ragged single block',
    64: 'exactly one block',
    65: 'second key block with one live key, second query block with one live row',
    127: 'the last length below the flash forward',
    128: 'threshold of the flash forward: two whole blocks, one `full` pair',
    129: 'flash forward; a third query block with one live row next to `full` ones',
    191: '`full` pair (1, 0) next to the ragged last query block',
    193: 'query blocks 1 and 2 against key block 0 are `full`, block 3 has one live row, the diagonal blocks are masked',
}
CROSS = {
    (2, 1): 'Lk = 1',
    (1, 33): 'Lq = 1',
    (70, 6): 'the slot cross-attention shape: ragged second query block, six keys',
    (64, 7): 'exactly one query block',
    (65, 64): 'one whole key block (`full` with query block 0), a query block with one live row',
    (130, 65): 'a key block with one live key',
    (129, 128): 'two whole key blocks, `full` next to a one-row query block',
    (257, 130): 'four `full` query blocks per whole key block, a one-row fifth, a two-key third key block',
}
B_CAUSAL, B_CROSS, HEADS = 2, 3, 2


def _table():
    rows = []

    def causal(L, hd, p=0., bwd=True, why=None):
        rows.append(Case(B_CAUSAL, HEADS, hd, L, L, True, p, bwd, why or CAUSAL_L[L]))

    def cross(Lq, Lk, hd, p=0., bwd=True, why=None):
        rows.append(Case(B_CROSS, HEADS, hd, Lq, Lk, False, p, bwd, why or CROSS[(Lq, Lk)]))

    # p = 0: every length and every cross shape meets hd 48 and one head dim of each generic width, the generic head dims in turn
    for i, L in enumerate(CAUSAL_L):
        for hd in (48, HD_W32[i % 5], HD_W64[i % 3]):
            causal(L, hd)
    for i, s in enumerate(CROSS):
        for hd in (48, HD_W32[i % 5], HD_W64[i % 3]):
            cross(*s, hd)
    # the head dims below 48 of the 48-wide kernel (clamped 16-byte loads, zeroed columns), each at a ragged causal length and a cross shape
    for L, hd in [(63, 36), (129, 40), (193, 44)]:
        causal(L, hd, why=f'hd {hd} zero-padded to 48; ' + CAUSAL_L[L])
    for s, hd in [((70, 6), 36), ((65, 64), 40), ((257, 130), 44)]:
        cross(*s, hd, why=f'hd {hd} zero-padded to 48; ' + CROSS[s])
    # head dims only the training forward takes; 18 and 50 at L >= 128 stay off the flash kernels
    for L, hd in [(65, 2), (129, 18), (193, 50)]:
        causal(L, hd, bwd=False, why=f'forward only, hd {hd}; ' + CAUSAL_L[L])
    for s, hd in [((70, 6), 2), ((64, 7), 18), ((130, 65), 50)]:
        cross(*s, hd, bwd=False, why=f'forward only, hd {hd}; ' + CROSS[s])
    # p = 0.1 on every kernel, causal and cross
    for L, hd in [(65, 16), (193, 32), (65, 48), (191, 40), (193, 48), (127, 60), (129, 64), (129, 16)]:
        causal(L, hd, 0.1, why='dropout 0.1; ' + CAUSAL_L[L])
    for s, hd in [((130, 65), 28), ((64, 7), 44), ((257, 130), 48), ((65, 64), 52), ((1, 33), 12)]:
        cross(*s, hd, 0.1, why='dropout 0.1; ' + CROSS[s])
    causal(65, 2, 0.1, bwd=False, why='forward only, hd 2, dropout 0.1')
    cross(130, 65, 50, 0.1, bwd=False, why='forward only, hd 50, dropout 0.1')
    # p = 0.5: rows whose live keys are all dropped (out = 0, zero gradient)
    rows.append(DROPPED_CAUSAL)
    rows.append(DROPPED_CROSS)
    rows.append(WORKLOAD)
    assert len(set(rows)) == len(rows)
    return rows


DROPPED_CAUSAL = Case(2, 2, 4, 65, 65, True, 0.5, True, 'dropout 0.5: fully dropped rows among the first queries')
DROPPED_CROSS = Case(3, 2, 48, 70, 6, False, 0.5, True, 'dropout 0.5 at the slot cross-attention shape: fully dropped rows')
WORKLOAD = Case(1, 1, 48, 1025, 1025, True, 0.1, True, "the workload's own head: the only long case")
CASES = _table()
BWD_CASES = [c for c in CASES if c.bwd]


def case_id(c):
    return f'{"causal" if c.causal else "cross"}-{c.Lq}x{c.Lk}-hd{c.hd}-p{c.p:g}'


def find(causal, Lq, Lk, hd, p):
    """the table's row of that shape (its B and H are the table's)"""
    hits = [c for c in CASES if (c.causal, c.Lq, c.Lk, c.hd, c.p) == (causal, Lq, Lk, hd, p)]
    assert len(hits) == 1, (causal, Lq, Lk, hd, p, hits)
    return hits[0]


# one case per kernel for the layout, repeat and independence tests: (case, what it is there for)
LAYOUT_CAUSAL = [find(True, 65, 65, 32, 0.), find(True, 193, 193, 44, 0.), find(True, 129, 129, 64, 0.1)]
LAYOUT_CROSS = [find(False, 130, 65, 28, 0.1), find(False, 70, 6, 36, 0.), find(False, 65, 64, 52, 0.1), DROPPED_CROSS]
INDEPENDENT = [find(True, 65, 65, 32, 0.), find(True, 193, 193, 44, 0.), find(False, 130, 65, 64, 0.)]   # p = 0, one per kernel


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def keep_mask(c):
    """bool [B, H, Lq, Lk], True = kept: element ((b*H + h)*Lq + q)*Lk + k of the attention-weight site's stream"""
    n = c.B * c.H * c.Lq * c.Lk
    if c.p == 0:
        return torch.ones(c.B, c.H, c.Lq, c.Lk, dtype=torch.bool)
    from slotformer_amd.train import dropout_keep_mask
    return torch.from_numpy(dropout_keep_mask(SEED, 0, 0, 0, n, c.p)).view(c.B, c.H, c.Lq, c.Lk)


def drop_scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def live_mask(c):
    """bool [Lq, Lk]: the pairs the causal mask leaves"""
    return ~torch.triu(torch.ones(c.Lq, c.Lk, dtype=torch.bool), 1) if c.causal else torch.ones(c.Lq, c.Lk, dtype=torch.bool)


def fully_dropped_rows(c):
    """number of (b, h, q) whose live keys are all dropped"""
    return int(((keep_mask(c) & live_mask(c)).sum(-1) == 0).sum())


def inputs(c):
    """the float32 tensors the kernels get: q [B,Lq,d], k, v [B,Lk,d] (those of steve_kernel_cases.attention_case), d_out [B,Lq,d]"""
    a = attention_case(c.B, c.H, c.hd, c.Lq, c.Lk, c.causal)
    return dict(q=a['q'], k=a['k'], v=a['v'], g=rnd(c.B, c.Lq, c.H * c.hd, seed=4), smax=a['smax'])


def attention(q, k, v, g, c, dtype):
    """autograd of the plain formula in `dtype` -> out, lse, dq, dk, dv"""
    B, H, hd = c.B, c.H, c.hd
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * hd**-0.5
    s = s.masked_fill(~live_mask(c), float('-inf'))
    att = torch.softmax(s, -1) * (keep_mask(c).to(dtype) * drop_scale(c.p))
    out = (att @ vh).transpose(1, 2).reshape(B, c.Lq, H * hd)
    out.backward(g.to(dtype))
    return dict(out=out.detach(), lse=torch.logsumexp(s, -1).detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def closed_form(q, k, v, g, c):
    """the kernels' own formulas in float64: dV = Pd^T dO, dP = dO V^T, D = rowsum(dO * O), dS = P (dP * mask - D),
    dK = dS^T (Q * scale), dQ = scale dS K"""
    B, H, hd, scale = c.B, c.H, c.hd, c.hd**-0.5
    Q, K, V, G = (t.double().view(B, -1, H, hd).transpose(1, 2) for t in (q, k, v, g))
    S = ((Q * scale) @ K.transpose(-1, -2)).masked_fill(~live_mask(c), float('-inf'))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    mask = keep_mask(c).double() * drop_scale(c.p)
    Pd = P * mask
    O = Pd @ V
    dV = Pd.transpose(-1, -2) @ G
    dP = G @ V.transpose(-1, -2)
    D = (G * O).sum(-1, keepdim=True)
    dS = P * (dP * mask - D)
    dK = dS.transpose(-1, -2) @ (Q * scale)
    dQ = scale * (dS @ K)
    # the size of the terms that dS = P (dP mask - D) subtracts, carried through the last products: see `floor_base`
    dS_abs = P * (dP.abs() * mask + D.abs())
    cancel = dict(dq=(scale * (dS_abs @ K.abs())).max().item(), dk=(dS_abs.transpose(-1, -2) @ (Q * scale).abs()).max().item())

    def rows(t):
        return t.transpose(1, 2).reshape(B, -1, H * hd)
    return dict(out=rows(O), lse=lse, dq=rows(dQ), dk=rows(dK), dv=rows(dV), cancel=cancel)


@functools.lru_cache(maxsize=None)
def reference64(c):
    """dict(out [B,Lq,d], lse [B,H,Lq], dq, dk, dv) in float64 by autograd, `closed` = the same from the closed form, and the inputs"""
    x = inputs(c)
    ref = attention(x['q'], x['k'], x['v'], x['g'], c, torch.float64)
    ref['closed'] = closed_form(x['q'], x['k'], x['v'], x['g'], c)
    ref.update(x)
    return ref


def floor_base(c, name):
    """None, or what the floor of the bound is taken from instead of max |reference|.  With a single key (Lk = 1) the softmax is the
    constant 1, dS = P (dP - D) is zero and so are dq and dk, exactly: max |reference| is 0 (or the 1e-16 that float64 leaves) and
    says nothing about the size of the rounding a correct kernel returns, which is that of the terms dS subtracts.  For these two
    outputs of these cases the floor is taken from max scale (P (|dP| mask + |D|)) |K| (for dk: ... ^T |Q| scale) instead."""
    return reference64(c)['closed']['cancel'][name] if c.Lk == 1 and name in ('dq', 'dk') else None


def ratio(a, b, tol, base=None):
    """largest |a - b| / (rtol |b| + floor max|b|) over all elements, as steve_kernel_cases.err_over_bound; base: see floor_base"""
    if base is None:
        return err_over_bound(a, b, tol)
    rtol, floor = tol
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs() / (rtol * b.abs() + floor * max(b.abs().max().item(), base))).max().item()


# ---------------------------------------------------------------------------------------------------------------------
# train._SelfAttention from its input: q | k | v = x [Wq; Wk; Wv]^T, then the causal attention with dropout
# ---------------------------------------------------------------------------------------------------------------------
# (four heads of 48: the packed projection's backward, sf_linear_bwd_f32, takes widths that are multiples of 64 only)
SELF_NODE = Case(2, 4, 48, 129, 129, True, 0.1, True, 'train._SelfAttention: causal L 129, dropout 0.1, width 192')
CROSS_NODE = find(False, 257, 130, 48, 0.1)


@functools.lru_cache(maxsize=None)
def self_attention_node_case():
    """x [B,L,d] ~ N(0,1), Wq, Wk, Wv [d,d] ~ N(0,1) / sqrt(d) (so that q, k, v are ~ N(0,1) again), d_out; float64 autograd ->
    out, dx, dwq, dwk, dwv"""
    c = SELF_NODE
    d = c.H * c.hd
    x, g = rnd(c.B, c.Lq, d, seed=21), rnd(c.B, c.Lq, d, seed=22)
    ws = [rnd(d, d, seed=23 + i, scale=d**-0.5) for i in range(3)]
    x64 = x.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    qh, kh, vh = ((x64 @ w.t()).view(c.B, -1, c.H, c.hd).transpose(1, 2) for w in w64)
    s = ((qh @ kh.transpose(-1, -2)) * c.hd**-0.5).masked_fill(~live_mask(c), float('-inf'))
    att = torch.softmax(s, -1) * (keep_mask(c).double() * drop_scale(c.p))
    out = (att @ vh).transpose(1, 2).reshape(c.B, c.Lq, d)
    out.backward(g.double())
    return dict(x=x, g=g, w=ws, out=out.detach(), dx=x64.grad, dw=[w.grad for w in w64])
