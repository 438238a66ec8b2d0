"""Case tables, float64 references and bounds of the encode lane's kernels -- the persistent first convolution (csrc/conv_first.hip), the
pixel-stationary per-pixel chain and its bf16-plane rows (csrc/pixel_mlp.hip), the Slot-Attention iteration on those rows (csrc/slot_chain.hip), the
one-launch slot prologue (csrc/slot_attn.hip) and the matrix-core slot update with the next step's prologue behind it (csrc/slot_update_mfma.hip) --
shared by tests/test_encode_kernel_cases.py (CPU) and tests/test_encode_kernels_gpu.py.  Plain torch on the CPU; the library is not imported here.

Every reference is computed in float64 from the float32 inputs the kernel gets, once per case (lru_cache): do not write into one.

Next to each reference stand two CPU evaluations of the same function in the arithmetic of the kernels' matrix products: an operand x travels as
hi = bf16(x), lo = bf16(x - hi) and a product is hi.hi + hi.lo + lo.hi (`split`: the lo.lo term dropped), or hi.hi alone (`single`: what a kernel
computes that loses its lo operand).  The products themselves are summed in float64.  A bound is worth asserting when `split` sits within half of it
and `single` breaks it (tests/test_encode_kernel_cases.py); neither is ever compared with a kernel.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def bf16_rne(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    return x.float().bfloat16().float()


def split(x):
    """float32 x -> (hi, lo) float32 tensors that hold bfloat16 values: hi = bf16(x), lo = bf16(x - hi)"""
    hi = bf16_rne(x)
    return hi, bf16_rne(x.float() - hi)


def planes_of(x):
    """float32 [..., C] -> bfloat16 [..., 2 C]: hi | lo, the 512-byte rows of the encode at C = 128"""
    hi, lo = split(x)
    return torch.cat([hi, lo], -1).bfloat16()


def product(op, a, b, mode):
    """op(a, b) for a bilinear op on float32 operands, evaluated in float64: exactly ('f64'), on split operands without lo.lo ('split'), on the hi
    operands alone ('single'), or in float32 ('f32')."""
    if mode == 'f64':
        return op(a.double(), b.double())
    if mode == 'f32':
        return op(a.float(), b.float()).double()
    (ah, al), (bh, bl) = split(a), split(b)
    out = op(ah.double(), bh.double())
    if mode == 'split':
        out = out + op(ah.double(), bl.double()) + op(al.double(), bh.double())
    else:
        assert mode == 'single', mode
    return out


def f32(x):
    """the float32 rounding between two stages of a kernel"""
    return x.float()


def over_abs_bound(a, ref, bound):
    """largest |a - ref| / bound; bound a tensor of ref's shape or a number"""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs() / bound).max().item()


def err_over_bound(a, b, tol):
    """largest |a - b| / (rtol |b| + floor max|b|) over the elements (tests/steve_kernel_cases.py)"""
    rtol, floor = tol
    b = torch.as_tensor(b).detach().cpu().double()
    return over_abs_bound(a, b, (rtol * b.abs() + floor * b.abs().max()).clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# first convolution.  conv_first_kernel: a tile = 2 output rows of a frame, 32 tiles per frame at either resolution; launch_cf gives it
# min(2 * sf_stream_cus(stream), tiles) workgroups, workgroup g walks tiles g, g + grid, ... with the next halo prefetched in registers.
# ---------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(64, 1), (128, 2)]               # (resolution, stride)
CONV_FRAMES = (1, 2, 3)                         # 32, 64, 96 tiles
CONV_CUS = (1, 3, 5, 0)                         # pretended CUs (grids 2, 6, 10: 16-48 tiles per workgroup, ragged at 32 / 6 and 96 / 10); 0: the whole chip
CONV_OPTIONS = [(True, True, True), (False, False, False), (True, True, False), (False, False, True)]   # (bias, relu, table): test_conv_mfma_shape_gpu.OPTIONS
CONV_RTOL = CONV_ATOL = 1e-4                    # max |err| <= 1e-4 + 1e-4 max |ref| (test_conv_mfma_shape_gpu)
CONV_CLIP = (2, 3)                              # [B, T] of the grouped case


@functools.lru_cache(maxsize=None)
def conv_case(res, stride, frames=3):
    """img [frames, 3, res, res], w [64, 3, 5, 5], bias [64], table [4096, 64] (the inputs of test_conv_first) and the float64 convolution without bias /
    ReLU / table, NHWC [frames, 64, 64, 64]"""
    img, w, b, add = rnd(frames, 3, res, res, seed=1), rnd(64, 3, 5, 5, seed=2, scale=0.1), rnd(64, seed=3, scale=0.1), rnd(4096, 64, seed=4)
    return dict(img=img, w=w, b=b, add=add, raw=conv_raw(img, w, stride, 'f64'))


def conv_raw(img, w, stride, mode):
    return product(lambda a, b: F.conv2d(a, b, None, stride=stride, padding=2), img, w, mode).permute(0, 2, 3, 1).contiguous()


def conv_finish(raw, c, bias, relu, table):
    """bias, ReLU and the table in float64 on a raw convolution [F, 64, 64, 64]"""
    out = raw + c['b'].double() if bias else raw
    if relu:
        out = torch.relu(out)
    return out + c['add'].double().view(1, 64, 64, 64) if table else out


def conv_over_bound(out, ref):
    err = (torch.as_tensor(out).detach().cpu().double() - ref).abs().max().item()
    return err / (CONV_ATOL + CONV_RTOL * ref.abs().max().item())


def conv_nonfinite_expected(bad, stride):
    """bad: boolean [F, 3, H, W] -> boolean NHWC-less [F, 64, 64]: the outputs whose 5 x 5 window (at the stride, padding 2) holds a marked input"""
    return F.conv2d(bad.double(), torch.ones(1, 3, 5, 5, dtype=torch.float64), None, stride=stride, padding=2)[:, 0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# per-pixel chain.  pixel_feat_tok_kernel: a tile = 32 pixels, 8 waves per workgroup, grid = min(ceil(tiles / 8), sf_stream_cus(stream)), wave w of
# workgroup g walks tiles 8 g + w, + 8 grid, ...: tpw = ceil(tiles / (8 grid)) rounds.
# ---------------------------------------------------------------------------------------------------------------------
PIXEL_CASES = [   # (pretended CUs, M)
    (1, 32 * 8 * 2 - 5),          # 16 tiles on 8 waves: tpw 2, ragged last tile
    (1, 32 * 8 * 3 - 5),          # 24 tiles: tpw 3, ragged last tile
    (1, 32 * (8 * 2 + 3) + 1),    # 20 tiles: tpw 3, the last one holds one pixel, waves 4-7 have no tile in the last round
    (3, 32 * 24 * 2 - 5),         # 48 tiles on 3 workgroups: tpw 2
    (3, 32 * (24 * 2 + 3) + 1),   # 52 tiles: tpw 3, workgroups 1 and 2 idle in the last round
    (0, 100),                     # the whole chip: one workgroup, waves 4-7 idle
]
# The bound of test_pixel_feat_forms is max |err| <= 1e-4 + 1e-4 max |ref| = 5e-4 on these outputs (LayerNorm outputs, max |ref| 4.1 - 4.5).  The split
# evaluation of these cases sits at 3.6e-5 -- two chained products of K = 64 and K = 128 whose operands keep 16 bits, through the last LayerNorm -- which left
# it 14x room.  Tightened to 1.5e-5 + 1.5e-5 max |ref| (7.7e-5 - 8.2e-5): the split evaluation uses 0.44 - 0.47 of it, the single-bf16 one breaks it 230x, and
# a float32 evaluation (the kernel's LayerNorms and accumulators) moves 0.02 of it.
PIXEL_RTOL = PIXEL_ATOL = 1.5e-5


@functools.lru_cache(maxsize=None)
def pixel_weights():
    """the weights of test_pixel_feat_forms: (ln0_g, ln0_b, w1, b1, w2, b2, ln1_g, ln1_b)"""
    return (1 + 0.1 * rnd(64, seed=2), 0.1 * rnd(64, seed=3), rnd(128, 64, seed=4, scale=0.15), 0.1 * rnd(128, seed=5),
            rnd(128, 128, seed=6, scale=0.1), 0.1 * rnd(128, seed=7), 1 + 0.1 * rnd(128, seed=8), 0.1 * rnd(128, seed=9))


def pixel_eval(x, mode):
    g0, b0, w1, bb1, w2, bb2, g1, b1 = pixel_weights()
    lin = lambda a, w: product(lambda p, q: p @ q.t(), a, w, mode)   # noqa: E731
    h = f32(F.layer_norm(x.double(), (64, ), g0.double(), b0.double()))
    h = f32(torch.relu(lin(h, w1) + bb1.double()))
    return F.layer_norm(lin(h, w2) + bb2.double(), (128, ), g1.double(), b1.double())


@functools.lru_cache(maxsize=None)
def pixel_case(M):
    x = rnd(M, 64, seed=1)
    return dict(x=x, ref=pixel_eval(x, 'f64'))


def pixel_over_bound(out, ref):
    err = (torch.as_tensor(out).detach().cpu().double() - ref).abs().max().item()
    return err / (PIXEL_ATOL + PIXEL_RTOL * ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# Slot-Attention iteration on bf16 hi | lo rows.  sa_attn_planes_kernel: one workgroup per 512 pixels of a frame, four waves of 128 pixels; the logits
# come out as [16 slot rows][pixels] with slots 0-3 in rows 0-3 and slots 4-7 in rows 8-11 (N <= 4: the second half holds -3e38 padding only).
# ---------------------------------------------------------------------------------------------------------------------
SA_D = 128
SA_SCALE = SA_D**-0.5
SA_EPS = 1e-6                    # SlotAttention.eps of the models
SA_GAINS = (1, 8, 32)            # q ~ gain * N(0, 1): logits of std gain, softmax from soft to near one-hot
SA_SLOTS = (1, 3, 4, 5, 7, 8)
SA_CASES = [(B, HW, N) for B in (1, 3) for HW in (512, 1024) for N in SA_SLOTS] + [(2, 4096, 7)]
SA_GAP_ROWS = 512                # NaN rows between frames in the strided form


@functools.lru_cache(maxsize=None)
def sa_frame(b, HW):
    """frame b's rows: x ~ N(0, 1) as planes [HW, 256] bfloat16 and x_rec = hi + lo (exact in float32) [HW, 128]; the same for every B"""
    planes = planes_of(rnd(HW, SA_D, seed=100 + b))
    return planes, planes[:, :SA_D].float() + planes[:, SA_D:].float()


@functools.lru_cache(maxsize=None)
def sa_queries(b, N, gain):
    return rnd(N, SA_D, seed=200 + 10 * b + N) * float(gain)


def sa_eval(x, q, mode):
    """one frame: x [HW, 128] float32 (hi + lo of the planes), q [N, 128] -> attn [N, HW], num [HW / 512, N, 128], den [HW / 512, N] in float64, the
    products in `mode`.  The kernel scales q by scale * log2(e) in float32 before it splits it and runs the softmax in base 2."""
    HW, N = x.shape[0], q.shape[0]
    if mode == 'f64':
        logits = SA_SCALE * (q.double() @ x.double().t())
    else:
        q2 = f32(q * (SA_SCALE * math.log2(math.e)))
        logits = product(lambda a, b: a @ b.t(), q2, x, mode) * math.log(2.)
    attn = torch.softmax(logits, 0)
    w = attn + SA_EPS
    wc, xc = (w if mode == 'f64' else f32(w)).view(N, HW // 512, 512).transpose(0, 1), x.view(HW // 512, 512, SA_D)
    num = product(lambda a, b: a @ b, wc, xc, mode)
    return attn, num, wc.double().sum(-1)


@functools.lru_cache(maxsize=None)
def sa_case(b, HW, N, gain):
    """frame b at (HW, N, gain): the float64 reference and the bounds.
      logits, in the kernel's base-2 units, per pixel and slot: delta <= 2^-16 scale log2(e) sum_c |q_c| |x_c| -- the residual of the split of q 2^-18, the
        dropped lo.lo term 2^-18, float32 accumulation over K = 128 2^-17
      attention: |da| <= 2 ln2 delta a (1 - a) + 2^-20, delta the largest over the pixel's slots (v_exp_f32 and v_rcp_f32: the last term)
      a record's numerator / denominator: that summed over the record's 512 pixels (weighted by |x|) + 2^-16 sum a |x| (the split of a) / + 2^-16 sum a"""
    planes, x = sa_frame(b, HW)
    q = sa_queries(b, N, gain)
    attn, num, den = sa_eval(x, q, 'f64')
    xd = x.double()
    delta = 2.**-16 * SA_SCALE * math.log2(math.e) * (q.double().abs() @ xd.abs().t())        # [N, HW]
    attn_bound = 2 * math.log(2.) * delta.max(0, keepdim=True)[0] * attn * (1 - attn) + 2.**-20
    ab, ac, xa = attn_bound.view(N, HW // 512, 512).transpose(0, 1), attn.view(N, HW // 512, 512).transpose(0, 1), xd.abs().view(HW // 512, 512, SA_D)
    num_bound = ab @ xa + 2.**-16 * (ac @ xa)
    den_bound = ab.sum(-1) + 2.**-16 * ac.sum(-1)
    return dict(planes=planes, x=x, q=q, attn=attn, num=num, den=den, attn_bound=attn_bound, num_bound=num_bound, den_bound=den_bound)


def sa_updates(num, den):
    """[..., chunks, N, 128], [..., chunks, N] -> updates [..., N, 128] = sum of the records' numerators / sum of their denominators"""
    return num.double().sum(-3) / den.double().sum(-2).unsqueeze(-1)


# ---------------------------------------------------------------------------------------------------------------------
# slot prologue.  sa_slot_prologue_kernel: SU_R = 8 rows per workgroup; exact float32.
# ---------------------------------------------------------------------------------------------------------------------
SLOT_TOL = (2e-5, 2e-5)          # |a - b| <= rtol |b| + floor max|b|: what test_kernels_gpu.close holds float32 kernels to
PROLOGUE_D = (64, 128, 192)
PROLOGUE_BN = [(1, 1), (1, 7), (8, 1), (9, 1), (7, 5), (5, 7)]    # R = B N = 1, 7, 8, 9, 35, 35: ragged against SU_R = 8, from N = 1, 5, 7
PROLOGUE_T = 3                   # noise and kernel_dist rows of a [B][T][N][..] buffer, step 1 of 3
PROLOGUE_LOGVAR = 2.0


@functools.lru_cache(maxsize=None)
def prologue_weights(D):
    """torch-layout weights of ResidualMLPPredictor (LN, Linear(D, 2D), ReLU, Linear(2D, D)), the kernel-distribution Linear(D, 2D) and project_q (LN,
    Linear(D, D) without bias), and init_latents for up to 7 slots"""
    s = 10 * D
    return dict(pm_ln_g=1 + 0.1 * rnd(D, seed=s + 1), pm_ln_b=0.1 * rnd(D, seed=s + 2), pm_w0=rnd(2 * D, D, seed=s + 3, scale=D**-0.5),
                pm_b0=0.1 * rnd(2 * D, seed=s + 4), pm_w2=rnd(D, 2 * D, seed=s + 5, scale=(2 * D)**-0.5), pm_b2=0.1 * rnd(D, seed=s + 6),
                kd_w=rnd(2 * D, D, seed=s + 7, scale=0.35 * D**-0.5), kd_b=0.1 * rnd(2 * D, seed=s + 8), q_ln_g=1 + 0.1 * rnd(D, seed=s + 9),
                q_ln_b=0.1 * rnd(D, seed=s + 10), q_w=rnd(D, D, seed=s + 11, scale=D**-0.5), init=rnd(7, D, seed=s + 12))


def prologue_eval(w, prev, init, noise, norm_first, mode):
    """savi.py:393-402 (prev None: the init_latents row of the slot), predictor.py:65-73, project_q.  prev [B, N, D] or None, init [N, D], noise [B, N, D]
    or None -> (kernel_dist [B, N, 2D], slots [B, N, D], q [B, N, D]) in float64"""
    D = w['q_w'].shape[0]
    lin = lambda a, m: product(lambda p, q: p @ q.t(), a, m, mode)   # noqa: E731
    cast = (lambda t: t.double()) if mode == 'f64' else (lambda t: f32(t).double())
    if prev is None:
        lat = init.double()[None]
    else:
        x = prev.double()
        ln = cast(F.layer_norm(x, (D, ), w['pm_ln_g'].double(), w['pm_ln_b'].double()))
        hid = cast(torch.relu(lin(ln, w['pm_w0']) + w['pm_b0'].double()))
        lat = cast(lin(hid, w['pm_w2']) + w['pm_b2'].double() + (ln if norm_first else x))
    kdist = cast(lin(lat, w['kd_w']) + w['kd_b'].double())
    slots = kdist[..., :D]
    if noise is not None:
        slots = slots + noise.double() * torch.exp(0.5 * kdist[..., D:])
    slots = cast(slots)
    q = lin(cast(F.layer_norm(slots, (D, ), w['q_ln_g'].double(), w['q_ln_b'].double())), w['q_w'])
    return kdist, slots, q


@functools.lru_cache(maxsize=None)
def prologue_case(D, B, N, with_prev, norm_first, with_noise):
    w = prologue_weights(D)
    init = w['init'][:N].contiguous()
    prev = rnd(B, N, D, seed=D + 31 * B + N) if with_prev else None
    noise = rnd(B, N, D, seed=D + 31 * B + N + 1) if with_noise else None
    kdist, slots, q = prologue_eval(w, prev, init, noise, norm_first, 'f64')
    assert kdist[..., D:].abs().max() <= PROLOGUE_LOGVAR, kdist[..., D:].abs().max()
    # (prev None: one row per slot, every video starts from the same latents)
    kdist, slots, q = kdist.expand(B, N, 2 * D), slots.expand(B, N, D), q.expand(B, N, D)
    return dict(w=w, init=init, prev=prev, noise=noise, kdist=kdist.contiguous(), slots=slots.contiguous(), q=q.contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# slot update on the matrix cores and its NEXT form.  sa_slot_update_mfma_kernel: 32 rows per workgroup, split-bf16 products; eight partial records in
# flight, a second round of eight for P > 8; p_step 2 reads records 0, 2, 4, ... only.
# ---------------------------------------------------------------------------------------------------------------------
UPDATE_D, UPDATE_H = 128, 256
UPDATE_CASES = [(1, 3, 4), (5, 7, 16), (9, 8, 16), (32, 7, 16)]   # (B, N, P): R = 3, 35, 72, 224 rows -- one ragged workgroup, 2, 3 (ragged), 7 full
UPDATE_TOL_SLOTS, UPDATE_TOL_Q = 3e-5, 5e-5    # max |err| <= tol + tol max |ref| (test_slot_update_on_the_matrix_cores)
NEXT_TOL = (5e-5, 5e-5)                        # |a - b| <= rtol |b| + floor max|b|: the encode's bar
UPDATE_T, UPDATE_HORIZON = 3, 2                # out2 rows of a [B][T + H][N][D] rollout buffer; noise / kernel_dist rows of [B][T][N][..]


@functools.lru_cache(maxsize=None)
def update_weights():
    """the weights of test_slot_update_on_the_matrix_cores (GRUCell, LayerNorm + MLP), torch layout"""
    D, H = UPDATE_D, UPDATE_H
    return dict(w_ih=rnd(3 * D, D, seed=5, scale=D**-0.5), w_hh=rnd(3 * D, D, seed=6, scale=D**-0.5), b_ih=rnd(3 * D, seed=7, scale=0.1),
                b_hh=rnd(3 * D, seed=8, scale=0.1), ln_g=1 + 0.1 * rnd(D, seed=9), ln_b=0.1 * rnd(D, seed=10), w1=rnd(H, D, seed=11, scale=D**-0.5),
                b1=rnd(H, seed=12, scale=0.1), w2=rnd(D, H, seed=13, scale=H**-0.5), b2=rnd(D, seed=14, scale=0.1))


def update_eval(u, pw, pn, pd, prev, mode):
    """savi.py:95-100 from the partial records pn [B, P, N, D], pd [B, P, N] and the previous slots [B, N, D] -> (slots, project_q(slots)) in float64;
    pw: prologue_weights(128) for project_q"""
    D = UPDATE_D
    lin = lambda a, m: product(lambda p, q: p @ q.t(), a, m, mode)   # noqa: E731
    cast = (lambda t: t.double()) if mode == 'f64' else (lambda t: f32(t).double())
    upd, h = cast(pn.double().sum(1) / pd.double().sum(1).unsqueeze(-1)), prev.double()
    gi, gh = lin(upd, u['w_ih']) + u['b_ih'].double(), lin(h, u['w_hh']) + u['b_hh'].double()
    r, z = torch.sigmoid(gi[..., :D] + gh[..., :D]), torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
    hn = cast((1 - z) * torch.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:]) + z * h)
    hid = cast(torch.relu(lin(cast(F.layer_norm(hn, (D, ), u['ln_g'].double(), u['ln_b'].double())), u['w1']) + u['b1'].double()))
    x = cast(hn + lin(hid, u['w2']) + u['b2'].double())
    return x, lin(cast(F.layer_norm(x, (D, ), pw['q_ln_g'].double(), pw['q_ln_b'].double())), pw['q_w'])


def update_next_eval(u, pw, pn, pd, prev, noise, norm_first, mode):
    """the update, then the slot prologue of the following step on its rows -> (slots, kernel_dist, next_slots, project_q(next_slots))"""
    x, _ = update_eval(u, pw, pn, pd, prev, mode)
    kdist, nxt, q = prologue_eval(pw, x if mode == 'f64' else f32(x), None, noise, norm_first, mode)
    return x, kdist, nxt, q


@functools.lru_cache(maxsize=None)
def update_case(B, N, P, p_step):
    """records as in test_slot_update_on_the_matrix_cores; p_step 2: the reference sums the even records, the odd ones are the caller's to poison"""
    D = UPDATE_D
    pn, pd, prev = rnd(B, P, N, D, seed=1), 0.5 + rnd(B, P, N, seed=2).abs(), rnd(B, N, D, seed=4)
    noise = rnd(B, N, D, seed=18)
    u, pw = update_weights(), prologue_weights(D)
    c = dict(pn=pn, pd=pd, prev=prev, noise=noise, u=u, pw=pw)
    c['slots'], c['q'] = update_eval(u, pw, pn[:, ::p_step], pd[:, ::p_step], prev, 'f64')
    for nf in (0, 1):
        for wn in (0, 1):
            c['next', nf, wn] = update_next_eval(u, pw, pn[:, ::p_step], pd[:, ::p_step], prev, noise if wn else None, nf, 'f64')[1:]
    return c
