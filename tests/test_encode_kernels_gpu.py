"""GPU parity of the encode lane's kernels, one C ABI call at a time, against float64 on the CPU: the persistent first convolution
(conv_first_kernel), the pixel-stationary per-pixel chain and its bf16 hi | lo rows (pixel_feat_tok_kernel), the Slot-Attention iteration on those rows
(sa_attn_planes_kernel), the one-launch slot prologue (sa_slot_prologue_kernel) and the matrix-core slot update with the next step's prologue behind it
(sa_slot_update_mfma_kernel<NEXT>).  tests/encode_kernel_cases.py holds the tables, the references and the bounds, tests/test_encode_kernel_cases.py
checks them on the CPU.

The persistent kernels size their grids by sf_stream_cus(stream).  A test that shrinks a grid runs on a torch.cuda.Stream() of its own for which
sf_stream_set_cus(stream, n) tells the library n CUs -- no hardware mask: a two-frame problem then walks 16 - 48 tiles per workgroup -- and forgets the
entry afterwards.  Every output buffer is filled with NaN and has a guard tail: every element a call owns must have been written, and the tail (and
every gap of a strided output) must still hold the bit pattern of the fill.
"""
import contextlib
import ctypes as C

import pytest
import torch

import encode_kernel_cases as ec

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 1024   # elements behind every output


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _err():
    return _lib().sf_last_error_string().decode()


@pytest.fixture(autouse=True)
def split_bf16_mode():
    assert _lib().sf_get_precision() == 1, 'the suite runs in the default split-bf16 mode'


def nan_like_bits(t):
    """True where the float32 / bfloat16 tensor still holds the bit pattern torch.full(..., nan) wrote"""
    bits = torch.int32 if t.dtype == torch.float32 else torch.int16
    return t.contiguous().view(bits) == torch.full((1, ), NAN, dtype=t.dtype).view(bits).item()


def filled(dev, n, dtype=torch.float32):
    return torch.full((n + GUARD, ), NAN, device=dev, dtype=dtype)


def owned(buf, n, what, all_written=True):
    """the n elements a call owns, on the CPU, after checking that the guard tail is untouched (and that all n were written)"""
    buf = buf.cpu()
    assert nan_like_bits(buf[n:]).all(), f'{what}: wrote behind its output'
    if all_written:
        left = int(nan_like_bits(buf[:n]).sum())
        assert left == 0, f'{what}: {left} of {n} elements never written'
    return buf[:n]


@contextlib.contextmanager
def on_cus(cus):
    """-> the stream handle for a C ABI call.  cus 0: torch's current stream (the whole chip).  Otherwise a stream of its own that the library believes
    to have `cus` CUs; it waits for what the current stream has queued (the uploads), is synchronised on the way out, and the entry is forgotten."""
    if cus == 0:
        yield torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        return
    lib = _lib()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    assert lib.sf_stream_set_cus(C.c_void_p(s.cuda_stream), cus) == 0
    try:
        assert lib.sf_stream_cus(C.c_void_p(s.cuda_stream)) == cus
        yield s.cuda_stream
        s.synchronize()
    finally:
        lib.sf_stream_set_cus(C.c_void_p(s.cuda_stream), 0)


def report(what, ratio):
    print(f'{what}: max err / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: max err / bound {ratio:.3f}'


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# 1. first convolution
# ---------------------------------------------------------------------------------------------------------------------
def conv_operands(dev, c):
    return {k: c[k].to(dev).contiguous() for k in ('w', 'b', 'add')}


def conv_call(dev, d, img, frame_stride, F_, res, stride, opt, cus, group=None, all_written=True):
    """img: a device tensor whose frame f starts f * frame_stride floats in (group = (fgroup, group_stride): the grouped entry) -> [F, 64, 64, 64] on the CPU"""
    bias, relu, table = opt
    n = F_ * 64 * 64 * 64
    out = filled(dev, n)
    with on_cus(cus) as st:
        args = (p(d['w']), p(d['b']) if bias else None, p(d['add']) if table else None, p(out), F_, 3, res, res, 64, 5, stride, int(relu), st)
        if group is None:
            rc = _lib().sf_conv2d_nchw_in_f32(p(img), frame_stride, *args)
        else:
            rc = _lib().sf_conv2d_nchw_in_grouped_f32(p(img), frame_stride, group[0], group[1], *args)
        assert rc == 0, _err()
    return owned(out, n, f'conv {res} F {F_} cus {cus}', all_written).view(F_, 64, 64, 64)


def with_gaps(img, dev):
    """[F, 3, H, W] -> a device buffer with a frame's worth of NaN behind every frame (frame stride 2 * 3 H W)"""
    buf = torch.full((img.shape[0], 2) + tuple(img.shape[1:]), NAN)
    buf[:, 0] = img
    return buf.to(dev)


@pytest.mark.parametrize('bias,relu,table', ec.CONV_OPTIONS)
@pytest.mark.parametrize('F_', ec.CONV_FRAMES)
@pytest.mark.parametrize('res,stride', ec.CONV_SHAPES)
def test_first_convolution_on_every_grid(dev, res, stride, F_, bias, relu, table):
    """conv_first_kernel through sf_conv2d_nchw_in_f32 against float64 on grids of 2, 6, 10 workgroups and the whole chip, frames contiguous and a NaN
    frame apart: the same bits on every grid"""
    c, opt = ec.conv_case(res, stride), (bias, relu, table)
    d = conv_operands(dev, c)
    ref = ec.conv_finish(c['raw'][:F_], c, *opt)
    img, gapped = c['img'][:F_].to(dev).contiguous(), with_gaps(c['img'][:F_], dev)
    whole = conv_call(dev, d, img, 3 * res * res, F_, res, stride, opt, 0)
    report(f'first conv {res} / {stride} F {F_} {opt} whole chip', ec.conv_over_bound(whole, ref))
    for cus in ec.CONV_CUS:
        for gap, src in ((1, img), (2, gapped)):
            out = conv_call(dev, d, src, gap * 3 * res * res, F_, res, stride, opt, cus)
            assert torch.equal(out, whole), (cus, gap, (out - whole).abs().max().item())


@pytest.mark.parametrize('res,stride', ec.CONV_SHAPES)
def test_first_convolution_of_a_clip_in_one_launch(dev, res, stride):
    """sf_conv2d_nchw_in_grouped_f32 on a [B = 2, T = 3] clip: output frame i is the convolution of clip[i % 2, i // 2], on every grid, with the bits of the
    ungrouped launch on the same frames"""
    B, T = ec.CONV_CLIP
    c = ec.conv_case(res, stride, B * T)
    d = conv_operands(dev, c)
    clip = c['img'].view(B, T, 3, res, res)                               # frame (b, t) = img[b * T + t]
    order = [(i % B) * T + i // B for i in range(B * T)]                  # output frame i
    gathered = c['img'][order].to(dev).contiguous()
    clip_dev, fe = clip.to(dev).contiguous(), 3 * res * res
    for opt in ec.CONV_OPTIONS:
        ref = ec.conv_finish(c['raw'][order], c, *opt)
        plain = conv_call(dev, d, gathered, fe, B * T, res, stride, opt, 0)
        for cus in ec.CONV_CUS:
            out = conv_call(dev, d, clip_dev, T * fe, B * T, res, stride, opt, cus, group=(B, fe))
            report(f'grouped first conv {res} / {stride} {opt} cus {cus}', ec.conv_over_bound(out, ref))
            assert torch.equal(out, plain), (cus, (out - plain).abs().max().item())


@pytest.mark.parametrize('res,stride', ec.CONV_SHAPES)
def test_first_convolution_keeps_non_finite_inputs_where_they_are(dev, res, stride):
    """One NaN in frame 0 and one inf in frame 2 come out non-finite at exactly the outputs whose 5 x 5 window (at the stride) holds them, on every grid: the
    halo a workgroup prefetches for its next tile carries nothing over.  No ReLU (its max would map a NaN to 0 by definition).  Every other output has the bits
    of the clean launch."""
    c, opt = ec.conv_case(res, stride), (True, False, False)
    d = conv_operands(dev, c)
    img = c['img'].clone()
    img[0, 1, res - 1, 3] = NAN                  # the last tile of frame 0: the next tile of any walk is in frame 1
    img[2, 0, 5 * stride, res - 1] = float('inf')
    expected = ec.conv_nonfinite_expected(~torch.isfinite(img), stride)
    assert expected[0].any() and expected[2].any() and not expected[1].any()
    clean = conv_call(dev, d, c['img'].to(dev).contiguous(), 3 * res * res, 3, res, stride, opt, 0)
    img = img.to(dev).contiguous()
    for cus in ec.CONV_CUS:
        out = conv_call(dev, d, img, 3 * res * res, 3, res, stride, opt, cus, all_written=False)
        bad = ~torch.isfinite(out)
        assert torch.equal(bad, expected[..., None].expand_as(bad)), (cus, int(bad.sum()), int(expected.sum()) * 64)
        assert torch.equal(out[~bad], clean[~bad]), cus


# ---------------------------------------------------------------------------------------------------------------------
# 2. per-pixel chain, forms 3 and 4
# ---------------------------------------------------------------------------------------------------------------------
def pixel_call(dev, x, form, cus):
    """sf_pixel_feat_f32 -> [M, 128] float32, or for form 4 [M, 256] bfloat16, on the CPU"""
    M = x.shape[0]
    w = [v.to(dev).contiguous() for v in ec.pixel_weights()]
    n, dtype = (M * 256, torch.bfloat16) if form == 4 else (M * 128, torch.float32)
    out = filled(dev, n, dtype)
    with on_cus(cus) as st:
        assert _lib().sf_pixel_feat_f32(p(x), *[p(v) for v in w], p(out), M, 1e-5, form, st) == 0, _err()
    return owned(out, n, f'pixel chain form {form} M {M} cus {cus}').view(M, -1)


@pytest.mark.parametrize('cus,M', ec.PIXEL_CASES)
def test_pixel_chain_walks_its_tiles(dev, cus, M):
    """pixel_feat_tok_kernel (form 3) where a wave walks two or three tiles, raggedly: against float64, the bits of the whole-chip launch, and nothing past
    row M"""
    c = ec.pixel_case(M)
    x = c['x'].to(dev).contiguous()
    out = pixel_call(dev, x, 3, cus)
    report(f'pixel chain form 3 M {M} cus {cus}', ec.pixel_over_bound(out, c['ref']))
    whole = pixel_call(dev, x, 3, 0)
    assert torch.equal(out, whole), (out - whole).abs().max().item()


@pytest.mark.parametrize('tok', (1, 0))
@pytest.mark.parametrize('cus,M', ec.PIXEL_CASES)
def test_pixel_chain_planes_are_the_split_of_the_f32_rows(dev, cus, M, tok):
    """form 4 (what the encode writes: the PLANES instantiation of the pixel-stationary kernel under sf_set_pixel_tok(1), of the streaming kernel under 0)
    is bit for bit hi = bf16(y), lo = bf16(y - hi) of the f32 rows y of form 3 / form 2 from the same launch geometry"""
    lib = _lib()
    c = ec.pixel_case(M)
    x = c['x'].to(dev).contiguous()
    old = lib.sf_get_pixel_tok()
    try:
        lib.sf_set_pixel_tok(tok)
        y = pixel_call(dev, x, 3 if tok else 2, cus)
        planes = pixel_call(dev, x, 4, cus)
    finally:
        lib.sf_set_pixel_tok(old)
    report(f'pixel chain form {3 if tok else 2} M {M} cus {cus}', ec.pixel_over_bound(y, c['ref']))
    expect = ec.planes_of(y)
    assert torch.equal(planes.view(torch.int16), expect.view(torch.int16)), int((planes.view(torch.int16) != expect.view(torch.int16)).sum())
    report(f'pixel chain form 4 (hi + lo) M {M} cus {cus}', ec.pixel_over_bound(planes[:, :128].double() + planes[:, 128:].double(), c['ref']))


# ---------------------------------------------------------------------------------------------------------------------
# 3. Slot-Attention iteration on bf16 hi | lo rows
# ---------------------------------------------------------------------------------------------------------------------
ATTN_PAD = 64   # floats between the attention maps of two frames


def planes_call(dev, frames, HW, N, gain, gap_rows, want_attn):
    """sf_slot_attn_iter_planes_f32 on the frames `frames` (ids of encode_kernel_cases.sa_frame), gap_rows NaN rows behind every frame
    -> part_num [B, P, N, 128], part_den [B, P, N], attn [B, N, HW] | None"""
    B, P, stride = len(frames), HW // 256, HW + gap_rows
    rows = torch.full((B * stride + 8, 256), NAN, dtype=torch.bfloat16)
    for i, b in enumerate(frames):
        rows[i * stride:i * stride + HW] = ec.sa_frame(b, HW)[0]
    rows = rows.to(dev)
    q = torch.stack([ec.sa_queries(b, N, gain) for b in frames]).to(dev).contiguous()
    pn, pd = filled(dev, B * P * N * 128), filled(dev, B * P * N)
    attn_bs = N * HW + ATTN_PAD
    attn = filled(dev, B * attn_bs) if want_attn else None
    assert _lib().sf_slot_attn_iter_planes_f32(p(rows), stride, p(q), p(pn), p(pd), p(attn), attn_bs, B, HW, N, ec.SA_SCALE, ec.SA_EPS,
                                               torch.cuda.current_stream().cuda_stream) == 0, _err()
    torch.cuda.synchronize()
    what = f'planes iteration B {B} HW {HW} N {N} gain {gain}'
    pn, pd = owned(pn, B * P * N * 128, what).view(B, P, N, 128), owned(pd, B * P * N, what).view(B, P, N)
    if attn is not None:
        attn = owned(attn, B * attn_bs, what, all_written=False).view(B, attn_bs)
        assert nan_like_bits(attn[:, N * HW:]).all(), f'{what}: wrote between two attention maps'
        attn = attn[:, :N * HW].reshape(B, N, HW)
        assert not nan_like_bits(attn).any(), what
    return pn, pd, attn


def tile_call(dev, frames, HW, N, gain):
    """the same rows as f32 through sf_slot_attn_iter_f32 with keys == values (the exact-f32 tile kernel at HW 4096) -> (sum of the numerators, of the
    denominators, attn)"""
    B, P = len(frames), _lib().sf_slot_attn_num_partials(HW)
    x = torch.stack([ec.sa_frame(b, HW)[1] for b in frames]).to(dev).contiguous()
    q = torch.stack([ec.sa_queries(b, N, gain) for b in frames]).to(dev).contiguous()
    pn, pd, attn = filled(dev, B * P * N * 128), filled(dev, B * P * N), filled(dev, B * N * HW)
    assert _lib().sf_slot_attn_iter_f32(p(x), p(x), 128, HW * 128, p(q), p(pn), p(pd), p(attn), B, HW, N, 128, ec.SA_SCALE, ec.SA_EPS,
                                        torch.cuda.current_stream().cuda_stream) == 0, _err()
    torch.cuda.synchronize()
    return (owned(pn, B * P * N * 128, 'tile').view(B, P, N, 128).double().sum(1), owned(pd, B * P * N, 'tile').view(B, P, N).double().sum(1),
            owned(attn, B * N * HW, 'tile').view(B, N, HW))


@pytest.mark.parametrize('B,HW,N', ec.SA_CASES)
def test_slot_attention_on_planes(dev, B, HW, N):
    """sa_attn_planes_kernel from soft to near one-hot attention: the records' layout, the derived bounds on attention, numerators and denominators per
    record, the same bits with and without attn_out / with NaN rows between the frames / whatever the batch.  Printed, not asserted: the attention and
    updates error of this kernel and of the exact-f32 kernel on the same rows (profiles/encode_kernel_tests.md)."""
    frames, P = list(range(B)), HW // 256
    for gain in ec.SA_GAINS:
        pn, pd, attn = planes_call(dev, frames, HW, N, gain, 0, True)
        assert pn.shape[1] == P
        assert (pn[:, 1::2] == 0).all() and (pd[:, 1::2] == 0).all(), 'the odd records are zero'
        cases = [ec.sa_case(b, HW, N, gain) for b in frames]
        what = f'planes iteration B {B} HW {HW} N {N} gain {gain}'
        report(f'{what} attention', max(ec.over_abs_bound(attn[b], c['attn'], c['attn_bound']) for b, c in enumerate(cases)))
        # record 2c: the sums over pixels 512 c .. 512 c + 511
        report(f'{what} numerators', max(ec.over_abs_bound(pn[b, 0::2], c['num'], c['num_bound']) for b, c in enumerate(cases)))
        report(f'{what} denominators', max(ec.over_abs_bound(pd[b, 0::2], c['den'], c['den_bound']) for b, c in enumerate(cases)))
        for gap, want in ((ec.SA_GAP_ROWS, True), (0, False), (ec.SA_GAP_ROWS, False)):
            pn2, pd2, attn2 = planes_call(dev, frames, HW, N, gain, gap, want)
            assert torch.equal(pn2, pn) and torch.equal(pd2, pd), (gap, want)
            assert attn2 is None or torch.equal(attn2, attn), gap
        if B > 1:   # a frame's records do not depend on the batch
            pn1, pd1, attn1 = planes_call(dev, [B - 1], HW, N, gain, 0, True)
            assert torch.equal(pn1[0], pn[B - 1]) and torch.equal(pd1[0], pd[B - 1]) and torch.equal(attn1[0], attn[B - 1])
        # ---- the figures of the record (not assertions) ----
        tn, td, tattn = tile_call(dev, frames, HW, N, gain)
        ref_attn, ref_upd = torch.stack([c['attn'] for c in cases]), torch.stack([ec.sa_updates(c['num'], c['den']) for c in cases])
        for name, a, u in (('planes', attn, ec.sa_updates(pn[:, 0::2], pd[:, 0::2])), ('f32 rows', tattn, tn / td.unsqueeze(-1))):
            print(f'MEASURED {what} {name}: attention max abs err {(a.double() - ref_attn).abs().max().item():.2e}, updates max abs err '
                  f'{(u - ref_upd).abs().max().item():.2e} (max |updates| {ref_upd.abs().max().item():.2f}, max attention {ref_attn.max().item():.4f})')


# ---------------------------------------------------------------------------------------------------------------------
# 4. slot prologue
# ---------------------------------------------------------------------------------------------------------------------
def strided_rows(dev, rows, T, step):
    """rows [B, N, W] or None -> (device buffer [B, T, N, W] of NaN with the rows at time step `step`, address of row (0, step), batch stride)"""
    if rows is None:
        return None, None, 0
    B, N, W = rows.shape
    buf = torch.full((B, T, N, W), NAN)
    buf[:, step] = rows
    buf = buf.to(dev)
    return buf, buf.data_ptr() + 4 * step * N * W, T * N * W


def strided_out(dev, B, T, N, W):
    buf = filled(dev, B * T * N * W)
    return buf


def read_strided(buf, B, T, N, W, step, what):
    """the rows of time step `step` of a [B, T, N, W] output; every other step and the guard still hold the fill"""
    full = owned(buf, B * T * N * W, what, all_written=False).view(B, T, N, W)
    rest = torch.ones(T, dtype=torch.bool)
    rest[step] = False
    assert nan_like_bits(full[:, rest]).all(), f'{what}: wrote outside its time step'
    assert not nan_like_bits(full[:, step]).any(), f'{what}: rows never written'
    return full[:, step]


@pytest.mark.parametrize('B,N', ec.PROLOGUE_BN)
@pytest.mark.parametrize('D', ec.PROLOGUE_D)
def test_slot_prologue(dev, D, B, N):
    """sa_slot_prologue_kernel against float64 of savi.py:393-402, predictor.py:65-73 and project_q, with row counts ragged against its eight rows per
    workgroup; noise and kernel_dist as step 1 of [B][3][N][..] buffers"""
    lib, T, step, R = _lib(), ec.PROLOGUE_T, 1, B * N
    w = ec.prologue_weights(D)
    dw = {k: (v.t() if k in ('pm_w0', 'pm_w2', 'kd_w', 'q_w') else v).contiguous().to(dev) for k, v in w.items()}
    for with_prev, norm_first in ((0, 0), (1, 0), (1, 1)):
        for with_noise in (0, 1):
            for with_kdist in (0, 1):
                c = ec.prologue_case(D, B, N, with_prev, norm_first, with_noise)
                what = f'prologue D {D} B {B} N {N} prev {with_prev} norm_first {norm_first} noise {with_noise} kdist {with_kdist}'
                prev = c['prev'].to(dev).contiguous() if with_prev else None
                init = c['init'].to(dev).contiguous()
                noise_buf, noise_ptr, noise_bs = strided_rows(dev, c['noise'], T, step)
                kd = strided_out(dev, B, T, N, 2 * D) if with_kdist else None
                slots, q = filled(dev, R * D), filled(dev, R * D)
                pm = [p(dw[k]) if with_prev else None for k in ('pm_ln_g', 'pm_ln_b', 'pm_w0', 'pm_b0', 'pm_w2', 'pm_b2')]
                rc = lib.sf_slot_prologue_f32(p(prev), p(init), *pm, norm_first, p(dw['kd_w']), p(dw['kd_b']), noise_ptr, noise_bs,
                                              kd.data_ptr() + 4 * step * N * 2 * D if with_kdist else None, T * N * 2 * D, p(dw['q_ln_g']), p(dw['q_ln_b']),
                                              p(dw['q_w']), p(slots), p(q), B, N, D, 1e-5, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, _err()
                torch.cuda.synchronize()
                r = [ec.err_over_bound(owned(slots, R * D, what).view(B, N, D), c['slots'], ec.SLOT_TOL),
                     ec.err_over_bound(owned(q, R * D, what).view(B, N, D), c['q'], ec.SLOT_TOL)]
                if with_kdist:
                    r.append(ec.err_over_bound(read_strided(kd, B, T, N, 2 * D, step, what), c['kdist'], ec.SLOT_TOL))
                report(what, max(r))


# ---------------------------------------------------------------------------------------------------------------------
# 5. slot update on the matrix cores, NEXT form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def update_operands(dev):
    """the packed matrices and the vectors of the update and of the next step's prologue, on the device"""
    from slotformer_amd import ops
    u, pw = ec.update_weights(), ec.prologue_weights(ec.UPDATE_D)
    d = {k: v.to(dev).contiguous() for k, v in list(u.items()) + list(pw.items())}
    for k in ('w_ih', 'w_hh', 'w1', 'w2', 'q_w', 'pm_w0', 'pm_w2', 'kd_w'):
        d[k + '_p'] = ops.pack_linear(d[k])
    torch.cuda.synchronize()
    return d


def update_call(dev, d, c, B, N, P, p_step, nxt=None):
    """sf_slot_update_packed_next_f32; nxt None: the plain form, else (norm_first, with_noise, with_kdist)
    -> dict(slots, out2, q[, next_slots, kdist]) on the CPU.  out2 is step 1 of a [B][T + H][N][D] rollout buffer, noise / kernel_dist step 2 of [B][T][N][..]."""
    D, H, R, T, TH = ec.UPDATE_D, ec.UPDATE_H, B * N, ec.UPDATE_T, ec.UPDATE_T + ec.UPDATE_HORIZON
    pn, pd = c['pn'].clone(), c['pd'].clone()
    if p_step == 2:
        # UmArgs.P (slot_update_body.h) documents which records are read: "records 0, pstep, 2 pstep, .. of the P * pstep the producer wrote" -- numerators
        # and denominators alike.  So the odd ones hold NaN here, not the producer's zeros: a read of one shows in every output.
        pn[:, 1::2], pd[:, 1::2] = NAN, NAN
    pn, pd, prev = pn.to(dev).contiguous(), pd.to(dev).contiguous(), c['prev'].to(dev).contiguous()
    slots, q, out2 = filled(dev, R * D), filled(dev, R * D), strided_out(dev, B, TH, N, D)
    nf, wn, wk = nxt if nxt is not None else (0, 0, 0)
    next_slots = filled(dev, R * D) if nxt is not None else None
    noise_buf, noise_ptr, noise_bs = strided_rows(dev, c['noise'] if wn else None, T, 2)
    kd = strided_out(dev, B, T, N, 2 * D) if wk else None
    rc = _lib().sf_slot_update_packed_next_f32(
        p(pn), p(pd), P, p(prev), p(d['w_ih_p']), p(d['w_hh_p']), p(d['b_ih']), p(d['b_hh']), p(d['ln_g']), p(d['ln_b']), p(d['w1_p']), p(d['b1']),
        p(d['w2_p']), p(d['b2']), p(slots), p(d['q_ln_g']), p(d['q_ln_b']), p(d['q_w_p']), p(q), B, N, D, H, 1e-5, out2.data_ptr() + 4 * N * D, TH * N * D,
        p_step, p(d['pm_ln_g']), p(d['pm_ln_b']), p(d['pm_w0_p']), p(d['pm_b0']), p(d['pm_w2_p']), p(d['pm_b2']), nf, p(d['kd_w_p']), p(d['kd_b']), noise_ptr,
        noise_bs, kd.data_ptr() + 4 * 2 * N * 2 * D if wk else None, T * N * 2 * D, p(next_slots), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _err()
    torch.cuda.synchronize()
    what = f'slot update B {B} N {N} P {P} p_step {p_step} next {nxt}'
    r = dict(slots=owned(slots, R * D, what).view(B, N, D), q=owned(q, R * D, what).view(B, N, D), out2=read_strided(out2, B, TH, N, D, 1, what))
    if nxt is not None:
        r['next_slots'] = owned(next_slots, R * D, what).view(B, N, D)
        if wk:
            r['kdist'] = read_strided(kd, B, T, N, 2 * D, 2, what)
    return r


@pytest.mark.parametrize('p_step', (1, 2))
@pytest.mark.parametrize('B,N,P', ec.UPDATE_CASES)
def test_slot_update_with_the_next_prologue(dev, update_operands, B, N, P, p_step):
    """sa_slot_update_mfma_kernel plain and NEXT against float64: the update's rows and q at the bounds of test_slot_update_on_the_matrix_cores, the next
    step's kernel_dist, sampled slots and q at the encode's 5e-5; slots_out and its strided copy hold the same bits, with and without NEXT"""
    c = ec.update_case(B, N, P, p_step)
    close = lambda a, b, t: ((a.double() - b).abs().max() / (t + t * b.abs().max())).item()   # noqa: E731
    what = f'slot update B {B} N {N} P {P} p_step {p_step}'
    plain = update_call(dev, update_operands, c, B, N, P, p_step)
    report(f'{what} slots', close(plain['slots'], c['slots'], ec.UPDATE_TOL_SLOTS))
    report(f'{what} q', close(plain['q'], c['q'], ec.UPDATE_TOL_Q))
    assert torch.equal(plain['out2'], plain['slots'])
    for nf in (0, 1):
        for wn in (0, 1):
            for wk in (0, 1):
                r = update_call(dev, update_operands, c, B, N, P, p_step, (nf, wn, wk))
                assert torch.equal(r['slots'], plain['slots']) and torch.equal(r['out2'], plain['slots']), (nf, wn, wk)
                kdist, nxt, q = c['next', nf, wn]
                ratios = [ec.err_over_bound(r['next_slots'], nxt, ec.NEXT_TOL), ec.err_over_bound(r['q'], q, ec.NEXT_TOL)]
                if wk:
                    ratios.append(ec.err_over_bound(r['kdist'], kdist, ec.NEXT_TOL))
                report(f'{what} next norm_first {nf} noise {wn} kdist {wk}', max(ratios))


# ---------------------------------------------------------------------------------------------------------------------
# the torch-tensor wrappers of slotformer_amd.ops over the same entry points (contiguous operands, torch's current stream)
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_wrappers(dev, update_operands):
    from slotformer_amd import ops
    # first convolution of a clip
    B, T = ec.CONV_CLIP
    c = ec.conv_case(64, 1, B * T)
    order = [(i % B) * T + i // B for i in range(B * T)]
    out = ops.conv2d_first_clip(c['img'].view(B, T, 3, 64, 64).to(dev), c['w'].to(dev), c['b'].to(dev), 1, relu=True, add=c['add'].to(dev))
    report('ops.conv2d_first_clip', ec.conv_over_bound(out, ec.conv_finish(c['raw'][order], c, True, True, True)))
    # per-pixel chain
    pc, w = ec.pixel_case(100), [v.to(dev) for v in ec.pixel_weights()]
    y = ops.pixel_feat(pc['x'].to(dev), w[0:2], w[2:4], w[4:6], w[6:8], form=3)
    report('ops.pixel_feat form 3', ec.pixel_over_bound(y, pc['ref']))
    planes = ops.pixel_feat(pc['x'].to(dev), w[0:2], w[2:4], w[4:6], w[6:8], form=4)
    assert planes.dtype == torch.bfloat16 and torch.equal(planes.cpu().view(torch.int16), ec.planes_of(y.cpu()).view(torch.int16))
    # Slot-Attention iteration on planes
    HW, N, gain = 1024, 7, 8
    cases = [ec.sa_case(b, HW, N, gain) for b in range(2)]
    pn, pd, attn = ops.slot_attn_iter_planes(torch.stack([s['planes'] for s in cases]).to(dev), torch.stack([s['q'] for s in cases]).to(dev),
                                             eps=ec.SA_EPS, want_attn=True)
    report('ops.slot_attn_iter_planes', max(max(ec.over_abs_bound(attn[b].cpu(), s['attn'], s['attn_bound']),
                                                ec.over_abs_bound(pn[b, 0::2].cpu(), s['num'], s['num_bound']),
                                                ec.over_abs_bound(pd[b, 0::2].cpu(), s['den'], s['den_bound'])) for b, s in enumerate(cases)))
    # slot prologue
    D, B, N = 128, 5, 7
    pw = {k: v.to(dev) for k, v in ec.prologue_weights(D).items()}
    pm, kd, q = [pw[k] for k in ('pm_ln_g', 'pm_ln_b', 'pm_w0', 'pm_b0', 'pm_w2', 'pm_b2')], (pw['kd_w'], pw['kd_b']), (pw['q_ln_g'], pw['q_ln_b'], pw['q_w'])
    s = ec.prologue_case(D, B, N, 1, 1, 1)
    out = ops.slot_prologue(s['prev'].to(dev), s['init'].to(dev), pm, kd, q, noise=s['noise'].to(dev), norm_first=True, want_kdist=True)
    report('ops.slot_prologue', max(ec.err_over_bound(a, b, ec.SLOT_TOL) for a, b in zip(out, (s['slots'], s['q'], s['kdist']))))
    s = ec.prologue_case(D, B, N, 0, 0, 0)
    out = ops.slot_prologue(None, s['init'].to(dev), None, kd, q, B=B)
    assert out[2] is None
    report('ops.slot_prologue from init_latents', max(ec.err_over_bound(a, b, ec.SLOT_TOL) for a, b in zip(out[:2], (s['slots'], s['q']))))
    # slot update + the next step's prologue
    B, N, P = 5, 7, 16
    u = ec.update_case(B, N, P, 2)
    d = update_operands
    pn, pd = u['pn'].clone(), u['pd'].clone()
    pn[:, 1::2], pd[:, 1::2] = NAN, NAN
    out = ops.slot_update_packed_next(pn.to(dev), pd.to(dev), u['prev'].to(dev), [d[k] for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')], d['ln_g'], d['ln_b'], d['w1'],
                                      d['b1'], d['w2'], d['b2'], q, pm, kd, noise=u['noise'].to(dev), norm_first=True, want_kdist=True, p_step=2)
    kdist, nxt, qn = u['next', 1, 1]
    report('ops.slot_update_packed_next slots', ((out[0].cpu().double() - u['slots']).abs().max() / (ec.UPDATE_TOL_SLOTS * (1 + u['slots'].abs().max()))).item())
    report('ops.slot_update_packed_next', max(ec.err_over_bound(a, b, ec.NEXT_TOL) for a, b in zip(out[1:], (nxt, qn, kdist))))
