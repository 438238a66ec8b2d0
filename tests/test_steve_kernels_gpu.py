"""GPU parity of the STEVE token-side forward kernels of csrc/steve_decoder.hip -- slate attention (flash, generic, K/V-cached decode,
training forward), the row-softmax family, arg-max, cross-entropy, token embedding, GroupNorm -- against float64 on the CPU, one C ABI
call at a time, at the sizes where the dispatch code or a kernel's own loop takes another path (tests/steve_kernel_cases.py holds the
tables and the references, tests/test_steve_kernel_cases.py checks them on the CPU).

Every comparison is element by element in the form of test_train_kernels_gpu.close: |a - b| <= rtol |b| + floor max|b|.
Arg-max rows that hold a NaN are unspecified (the winner depends on the order in which the threads merge) and nothing is asserted
for them; a row whose maximum is -inf returns its first index, as torch.argmax does.
"""
import pytest
import torch

import steve_kernel_cases as sc

pytestmark = pytest.mark.gpu

NAN = float('nan')


def close(a, b, tol, what, keep=None, per_row=False):
    ratio = sc.err_over_bound(a, b, tol, keep, per_row)
    print(f'{what}: max err / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: max err / bound {ratio:.3f}'
    return ratio


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().sf_last_error_string().decode()


def nan_like_bits(t):
    """True where the float32 tensor still holds the bit pattern torch.full(..., nan) wrote"""
    return t.contiguous().view(torch.int32) == torch.full((1, ), NAN).view(torch.int32).item()


# ---------------------------------------------------------------------------------------------------------------------
# slate attention
# ---------------------------------------------------------------------------------------------------------------------
def attn_call(q, k, v, out, ld, bs, B, Lq, Lk, H, hd, causal):
    """q, k, v, out: device addresses; ld = (ldq, ldk, ldv, ldo), bs = the four batch strides"""
    return _lib().sf_slate_attention_strided_f32(q, k, v, out, *ld, *bs, B, Lq, Lk, H, hd, int(causal), _stream())


def attn_contiguous(dev, c, H, causal, b=None):
    """the case's q, k, v as three contiguous tensors (of batch entry b alone) -> out [B, Lq, d]"""
    q, k, v = (c[n] if b is None else c[n][b:b + 1] for n in 'qkv')
    q, k, v = q.to(dev).contiguous(), k.to(dev).contiguous(), v.to(dev).contiguous()
    B, Lq, d = q.shape
    Lk = k.shape[1]
    out = torch.full((B, Lq, d), NAN, device=dev)
    assert attn_call(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), (d, d, d, d), (Lq * d, Lk * d, Lk * d, Lq * d), B, Lq, Lk,
                     H, d // H, causal) == 0, _err()
    return out.cpu()


def attn_side_by_side(dev, c, H, causal, pad_cols=0, out_extra=0):
    """q | k | v side by side in rows of 3 d + pad_cols floats of one buffer of max(Lq, Lk) + 7 rows per sequence, addressed with
    explicit batch strides; a single query sits in the row of the newest key, as in generation.  Everything the call has no business
    reading is NaN: the rows past Lq / Lk, the q columns of the other rows, the pad columns.  -> the whole output [B, Lq, d + out_extra]"""
    B, Lq, d = c['q'].shape
    Lk = c['k'].shape[1]
    rows, ld = max(Lq, Lk) + sc.CACHE_SPARE_ROWS, 3 * d + pad_cols
    q0 = Lk - 1 if Lq == 1 else 0
    buf = torch.full((B, rows, ld), NAN)
    buf[:, q0:q0 + Lq, :d], buf[:, :Lk, d:2 * d], buf[:, :Lk, 2 * d:3 * d] = c['q'], c['k'], c['v']
    buf = buf.to(dev)
    out = torch.full((B, Lq, d + out_extra), NAN, device=dev)
    p = buf.data_ptr()
    assert attn_call(p + 4 * q0 * ld, p + 4 * d, p + 8 * d, out.data_ptr(), (ld, ld, ld, d + out_extra),
                     (rows * ld, rows * ld, rows * ld, Lq * (d + out_extra)), B, Lq, Lk, H, d // H, causal) == 0, _err()
    return out.cpu()


@pytest.mark.parametrize('L,hd', sc.FLASH_CASES)
def test_flash_causal(dev, precision, L, hd):
    """slate_flash_bf3_kernel (bf16x3) / slate_flash_kernel (f32) at the tile edges"""
    c = sc.attention_case(2, 3, hd, L, L, True)
    close(attn_contiguous(dev, c, 3, True), c['out'], sc.TOL[precision], f'flash {precision} L {L} hd {hd}')


@pytest.mark.parametrize('L,hd', sc.GENERIC_CAUSAL_CASES)
def test_generic_causal(dev, L, hd):
    """slate_attn_kernel with the causal mask, below the flash threshold"""
    c = sc.attention_case(2, 3, hd, L, L, True)
    close(attn_contiguous(dev, c, 3, True), c['out'], sc.TOL_ATTN_F32, f'generic causal L {L} hd {hd}')


@pytest.mark.parametrize('Lq,Lk,hd', sc.GENERIC_CROSS_CASES)
def test_generic_cross(dev, Lq, Lk, hd):
    """slate_attn_kernel without a mask: the cross-attention to the slots, and Lq past one workgroup"""
    c = sc.attention_case(3, 2, hd, Lq, Lk, False)
    close(attn_contiguous(dev, c, 2, False), c['out'], sc.TOL_ATTN_F32, f'generic cross Lq {Lq} Lk {Lk} hd {hd}')


@pytest.mark.parametrize('Lk,hd', sc.DECODE_CASES)
def test_decode_over_a_cache(dev, Lk, hd):
    """slate_decode_attn_kernel on the first Lk rows of a cache of Lk + 7 rows of q | k | v, the way sf_slate_generate_f32 calls it"""
    c = sc.attention_case(3, 2, hd, 1, Lk, False)
    close(attn_side_by_side(dev, c, 2, False), c['out'], sc.TOL_ATTN_F32, f'decode Lk {Lk} hd {hd}')


def poison_check(dev, tol, B, H, Lq, Lk, hd, causal):
    """NaN in every row past Lq / Lk, in the pad columns of the side-by-side rows and all over an output of leading dimension d + 8:
    the d result columns hold no NaN and equal the contiguous call bit for bit, the 8 extra columns still hold the fill.  This reads
    and writes only memory the test owns."""
    c = sc.attention_case(B, H, hd, Lq, Lk, causal)
    d = H * hd
    out = attn_side_by_side(dev, c, H, causal, pad_cols=4, out_extra=8)
    res, extra = out[..., :d], out[..., d:]
    assert not torch.isnan(res).any()
    assert nan_like_bits(extra).all()
    assert torch.equal(res, attn_contiguous(dev, c, H, causal))
    close(res, c['out'], tol, f'poisoned Lq {Lq} Lk {Lk} hd {hd}')


@pytest.mark.parametrize('L,hd', [(193, 32), (129, 48)])
def test_flash_touches_nothing_past_the_sequence_or_the_row(dev, precision, L, hd):
    poison_check(dev, sc.TOL[precision], 2, 3, L, L, hd, True)


@pytest.mark.parametrize('Lq,Lk,hd,causal', [(70, 70, 48, True), (70, 6, 16, False), (257, 130, 64, False)])
def test_generic_touches_nothing_past_the_sequence_or_the_row(dev, Lq, Lk, hd, causal):
    poison_check(dev, sc.TOL_ATTN_F32, 3, 2, Lq, Lk, hd, causal)


@pytest.mark.parametrize('Lk,hd', [(65, 64), (257, 16)])
def test_decode_touches_nothing_past_the_sequence_or_the_row(dev, Lk, hd):
    poison_check(dev, sc.TOL_ATTN_F32, 3, 2, 1, Lk, hd, False)


def independence_check(dev, Lq, Lk, hd, causal):
    """entry b of a batch of 3 is bit-identical to the same sequence run alone"""
    c = sc.attention_case(3, 2, hd, Lq, Lk, causal)
    whole = attn_contiguous(dev, c, 2, causal)
    for b in range(3):
        assert torch.equal(whole[b:b + 1], attn_contiguous(dev, c, 2, causal, b)), b


def test_flash_sequences_of_a_batch_do_not_see_each_other(dev, precision):
    independence_check(dev, 191, 191, 64, True)


@pytest.mark.parametrize('Lq,Lk,hd,causal', [(65, 65, 32, True), (130, 65, 16, False), (1, 257, 48, False)])
def test_sequences_of_a_batch_do_not_see_each_other(dev, Lq, Lk, hd, causal):
    """the generic kernel with and without the mask, and the decode kernel"""
    independence_check(dev, Lq, Lk, hd, causal)


TRAIN_ULPS = 4


@pytest.mark.parametrize('L,hd', sc.TRAIN_FWD_CASES)
def test_training_forward_without_dropout(dev, precision, L, hd):
    """sf_slate_attention_train_fwd_f32 with p = 0.  L >= 128: the flash kernels' TRAIN instantiation.  It runs the arithmetic of the
    inference instantiation, but the two are compiled apart and `out` is NOT bit-identical: the compiler forms the final scale
    fw / (l fw + l_o fo) differently where the TRAIN form also needs the denominator for lse, and about 7 % of the elements differ in
    the last bit (largest difference measured 1.2e-7 at max |out| 2.9).  What holds is agreement to TRAIN_ULPS = 4 ulp of the largest
    output -- one for the scale, one for its product with each of the two key halves' partial outputs, one for their sum -- which is
    asserted, next to the precision mode's bound against float64.  L < 128: slate_attn_fwd_train_kernel, another kernel than the
    inference path's slate_attn_kernel (MFMA tiles, split-bf16 in that mode), held to the mode's bound against float64 only.
    lse against the float64 log-sum-exp, absolutely: rtol max|score| + floor."""
    B, H = 2, 3
    c = sc.attention_case(B, H, hd, L, L, True)
    d = H * hd
    q, k, v = (c[n].to(dev) for n in 'qkv')
    out, lse = torch.full((B, L, d), NAN, device=dev), torch.full((B, H, L), NAN, device=dev)
    assert _lib().sf_slate_attention_train_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), d, d, d, d,
                                                   L * d, L * d, L * d, L * d, B, L, L, H, hd, 1, 0.0, 0, _stream()) == 0, _err()
    rtol, floor = sc.TOL[precision]
    close(out, c['out'], sc.TOL[precision], f'train fwd {precision} L {L} hd {hd} out')
    if L >= 128:
        close(out, attn_contiguous(dev, c, H, True).double(), (0., TRAIN_ULPS * 2.**-23), 'against the inference call')
    err, bound = (lse.cpu().double() - c['lse']).abs().max().item(), rtol * c['smax'] + floor
    print(f'train fwd {precision} L {L} hd {hd} lse: max err / bound {err / bound:.3f}')
    assert not torch.isnan(lse).any() and err <= bound, (err, bound)


def test_refusals_leave_the_output_alone(dev):
    """head dim 24, causal with Lq != Lk, a leading dimension that is no multiple of 4: an error code, a message, an untouched output"""
    B, H = 2, 2

    def refused(hd, Lq, Lk, causal, ldo_extra, word):
        d = H * hd
        q, k, v = sc.rnd(B, Lq, d, seed=1).to(dev), sc.rnd(B, Lk, d, seed=2).to(dev), sc.rnd(B, Lk, d, seed=3).to(dev)
        out = torch.full((B, Lq, d + ldo_extra), NAN, device=dev)
        rc = attn_call(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), (d, d, d, d + ldo_extra),
                       (Lq * d, Lk * d, Lk * d, Lq * (d + ldo_extra)), B, Lq, Lk, H, hd, causal)
        torch.cuda.synchronize()
        assert rc != 0 and word in _err(), (rc, _err())
        assert nan_like_bits(out).all()

    for Lq, Lk, causal in [(1, 9, False), (9, 9, True), (200, 200, True), (9, 5, False)]:   # every dispatch arm ends in the refusal
        refused(24, Lq, Lk, causal, 0, 'head_dim')
    refused(16, 9, 7, True, 0, 'Lq == Lk')
    refused(16, 130, 131, True, 0, 'Lq == Lk')
    refused(16, 9, 9, True, 2, 'multiples of 4')
    refused(16, 1, 9, False, 2, 'multiples of 4')


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
def dev_rows(dev, t, offset=0, fill=None):
    """t (or, with fill, an array of t's shape holding `fill`) on the device, `offset` floats into its allocation"""
    flat = torch.full((t.numel() + 4, ), NAN if fill is None else fill, device=dev)
    view = flat[offset:offset + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset
    return view


def softmax_call(dev, x, add, scale, off=(0, 0, 0)):
    R, V = x.shape
    xd, ad = dev_rows(dev, x, off[0]), (dev_rows(dev, add, off[1]) if add is not None else None)
    y = dev_rows(dev, x, off[2], fill=NAN)
    assert _lib().sf_softmax_rows_f32(xd.data_ptr(), ad.data_ptr() if ad is not None else None, scale, y.data_ptr(), R, V, _stream()) == 0, _err()
    return y.cpu()


def log_softmax_call(dev, x, off=(0, 0)):
    xd, y = dev_rows(dev, x, off[0]), dev_rows(dev, x, off[1], fill=NAN)
    assert _lib().sf_log_softmax_rows_f32(xd.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], _stream()) == 0, _err()
    return y.cpu()


def softmax_bwd_call(dev, y, dy, scale, off=(0, 0, 0)):
    yd, gd, dx = dev_rows(dev, y, off[0]), dev_rows(dev, dy, off[1]), dev_rows(dev, y, off[2], fill=NAN)
    assert _lib().sf_softmax_rows_bwd_f32(yd.data_ptr(), gd.data_ptr(), scale, dx.data_ptr(), y.shape[0], y.shape[1], _stream()) == 0, _err()
    return dx.cpu()


@pytest.mark.parametrize('V', list(sc.ROW_V))
def test_softmax_rows(dev, V):
    """sf_softmax_rows_f32 with and without `add` at scale 1 and 10, sf_log_softmax_rows_f32, sf_softmax_rows_bwd_f32: reg<1>, reg<4>
    and the generic form on either side of each switch"""
    for with_add, scale in sc.SOFTMAX_FORMS:
        c = sc.softmax_case(V, with_add, scale)
        y = softmax_call(dev, c['x'], c['add'], scale)
        close(y, c['ref'], sc.TOL_ROWS, f'softmax V {V} add {with_add} scale {scale}')
        assert (y.double().sum(-1) - 1).abs().max() < 1e-5
    c = sc.softmax_case(V, False, 1.0, True)
    close(log_softmax_call(dev, c['x']), c['ref'], sc.TOL_ROWS, f'log_softmax V {V}')
    for scale in (1.0, 10.0):
        c = sc.softmax_bwd_case(V, scale)
        close(softmax_bwd_call(dev, c['y'], c['dy'], scale), c['ref'], sc.TOL_ROWS, f'softmax backward V {V} scale {scale}')


@pytest.mark.parametrize('which', [0, 1, 2])
def test_rows_off_alignment_take_the_generic_kernel(dev, which):
    """V = 1024 with x, add or y (y, dy or dx) 4 bytes into its allocation: the generic kernels, which sum in another order -- the same
    bound against float64, and the aligned call's result within that bound too"""
    V, off = 1024, tuple(int(i == which) for i in range(3))
    c = sc.softmax_case(V, True, 10.0)
    y0, y1 = softmax_call(dev, c['x'], c['add'], 10.0), softmax_call(dev, c['x'], c['add'], 10.0, off)
    close(y1, c['ref'], sc.TOL_ROWS, f'softmax, pointer {which} off by 4 bytes')
    close(y1, y0.double(), sc.TOL_ROWS, 'against the aligned call')
    b = sc.softmax_bwd_case(V, 10.0)
    d0, d1 = softmax_bwd_call(dev, b['y'], b['dy'], 10.0), softmax_bwd_call(dev, b['y'], b['dy'], 10.0, off)
    close(d1, b['ref'], sc.TOL_ROWS, f'softmax backward, pointer {which} off by 4 bytes')
    close(d1, d0.double(), sc.TOL_ROWS, 'against the aligned call')
    if which != 1:
        lg = sc.softmax_case(V, False, 1.0, True)
        close(log_softmax_call(dev, lg['x'], (off[0], off[2])), lg['ref'], sc.TOL_ROWS, f'log_softmax, pointer {which} off by 4 bytes')


@pytest.mark.parametrize('V', list(sc.LARGE_LOGIT_V))
def test_softmax_large_logits(dev, V):
    """max |z| = 300 after scaling.  The rounding of z, 2^-24 |z| per operation, reaches exp(z - max) undamped, so the fixed 1e-5 does
    not describe these rows: the kernel is allowed four times the error of float32 torch's CPU softmax on the same inputs (which
    rounds them once, where the kernel adds, scales and subtracts before expf) plus the ordinary bound.  Both are measured in units of
    that bound, with the floor taken from the element's own row."""
    c = sc.large_logit_case(V)
    for what, y, ref, t32 in [('softmax', softmax_call(dev, c['x'], c['add'], c['scale']), c['ref'], c['t32']),
                              ('log_softmax', log_softmax_call(dev, c['x_log']), c['ref_log'], c['t32_log'])]:
        e32, ek = sc.err_over_bound(t32, ref, sc.TOL_ROWS, per_row=True), sc.err_over_bound(y, ref, sc.TOL_ROWS, per_row=True)
        print(f'large logits V {V} {what}: err / bound, float32 torch {e32:.3f}, kernel {ek:.3f}, allowed {4 * e32 + 1:.3f}')
        assert torch.isfinite(y).all() and ek <= 4 * e32 + 1, (what, ek, e32)
    assert softmax_call(dev, c['x'], c['add'], c['scale'])[0, 7 % V] == 1.0   # the dominant entry


@pytest.mark.parametrize('V,R', sc.XENT_CASES)
def test_cross_entropy_forward(dev, V, R):
    """xent_rows_kernel + mean_kernel: rows to rtol 1e-5 + 1e-6, the mean (accumulated in double) to 1e-6 of the float64 mean"""
    c = sc.xent_case(V, R)
    x, tgt = c['x'].to(dev), c['tgt'].to(dev)
    rows, mean = torch.full((R, ), NAN, device=dev), torch.full((1, ), NAN, device=dev)
    assert _lib().sf_cross_entropy_f32(x.data_ptr(), tgt.data_ptr(), rows.data_ptr(), mean.data_ptr(), R, V, _stream()) == 0, _err()
    err = (rows.cpu().double() - c['rows']).abs()
    ratio = (err / (sc.XENT_RTOL * c['rows'].abs() + sc.XENT_ATOL)).max().item()
    merr, mbound = abs(mean.cpu().double().item() - c['mean'].item()), sc.XENT_MEAN_RTOL * abs(c['mean'].item())
    print(f'cross-entropy V {V} R {R}: rows err / bound {ratio:.3f}, mean err {merr:.3e} (bound {mbound:.3e})')
    assert ratio <= 1.0 and merr <= mbound, (ratio, merr, mbound)


@pytest.mark.parametrize('V', sc.ARGMAX_V)
def test_argmax_first_index_wins(dev, V):
    """ties inside one thread's strided slice, between two lanes, between two waves; the maximum at either end; rows of -inf.
    ld = V + 3 with +inf in the columns past V: a read past the row would win."""
    c = sc.argmax_case(V)
    R, ld = c['x'].shape[0], V + sc.ARGMAX_LD_EXTRA
    x = torch.full((R, ld), float('inf'))
    x[:, :V] = c['x']
    x = x.to(dev)
    out = torch.full((R, ), -1, dtype=torch.int64, device=dev)
    assert _lib().sf_argmax_rows_f32(x.data_ptr(), ld, out.data_ptr(), R, V, _stream()) == 0, _err()
    got = out.cpu().tolist()
    for r, (what, _, expected) in enumerate(c['table']):
        assert got[r] == expected, (V, what, got[r], expected)
    assert got == c['expected'].tolist()


@pytest.mark.parametrize('B,L,d,rows', sc.EMBED_CASES)
def test_embed_tokens_exact(dev, B, L, d, rows):
    c = sc.embed_case(B, L, d, rows)
    idx, emb, pos = c['idx'].to(dev), c['emb'].to(dev), c['pos'].to(dev)
    out = torch.full((B, L, d), NAN, device=dev)
    assert _lib().sf_embed_tokens_f32(idx.data_ptr(), emb.data_ptr(), pos.data_ptr(), out.data_ptr(), B, L, d, _stream()) == 0, _err()
    assert torch.equal(out.cpu(), c['ref'])


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm(1 group) (+ ReLU, + PixelShuffle)
# ---------------------------------------------------------------------------------------------------------------------
def groupnorm_call(dev, c, relu, shuffle):
    x, g, b = c['x'].to(dev), c['g'].to(dev), c['b'].to(dev)
    F_, H, W, C = x.shape
    y = torch.full(tuple(c['ref'].shape), NAN, device=dev)
    nb = _lib().sf_groupnorm1_workspace_bytes(F_)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert _lib().sf_groupnorm1_nhwc_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), F_, H, W, C, 1e-5, int(relu), shuffle,
                                         ws.data_ptr(), nb, _stream()) == 0, _err()
    return y.cpu()


@pytest.mark.parametrize('F_,H,W,C,shuffle,relu', sc.GN_CASES)
def test_groupnorm(dev, F_, H, W, C, shuffle, relu):
    """samples smaller than the 64 partial slices, H != W under the pixel shuffle, a slice length that does not divide; the elements
    within 1e-6 of the ReLU kink (none to a handful: test_steve_kernel_cases) are left out"""
    c = sc.groupnorm_case(F_, H, W, C, shuffle, relu)
    y = groupnorm_call(dev, c, relu, shuffle)
    assert not torch.isnan(y).any()
    close(y, c['ref'], sc.TOL_GN, f'groupnorm {(F_, H, W, C)} shuffle {shuffle} relu {relu}', ~c['excluded'])


@pytest.mark.parametrize('ratio', sc.GN_COND_RATIOS)
def test_groupnorm_mean_next_to_the_spread(dev, ratio):
    """x = ratio + N(0, 1): var = E[x^2] - mean^2 loses about ratio^2 of the precision of the float sums under it"""
    c = sc.groupnorm_case(*sc.GN_COND_SHAPE, 1, False, ratio)
    close(groupnorm_call(dev, c, False, 1), c['ref'], sc.TOL_GN, f'groupnorm mean / std {ratio}')


def test_groupnorm_conditioning_limit_is_measured(dev):
    """mean / std = 32, the documented limit (profiles/steve_kernel_tests.md): printed, not asserted"""
    c = sc.groupnorm_case(*sc.GN_COND_SHAPE, 1, False, sc.GN_COND_LIMIT)
    y = groupnorm_call(dev, c, False, 1)
    print(f'groupnorm mean / std {sc.GN_COND_LIMIT}: max err / bound {sc.err_over_bound(y, c["ref"], sc.TOL_GN):.3f}')
    assert torch.isfinite(y).all()
