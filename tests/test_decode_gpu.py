"""StoSAVi.decode / sf_savi_decode_seg_f32 and the kernels beside it against float64, on every branch the host code can take
(tests/decode_cases.py), with weights under which the segmentation rule of vp_utils.postproc_mask really decides something; the
recombination, segmentation and fragment-deconvolution entry points on crafted inputs."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_cases as dc
import oracle
from test_train_kernels_gpu import TOL, close

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(name, dev):
    if name not in _MODELS:
        _MODELS[name] = dc.build_case(name)[0].to(dev)
    return _MODELS[name]


def rel(a, b):
    a, b = a.detach().cpu().double(), b.double()
    return ((a - b).abs().max() / b.abs().max()).item()


def check_against_float64(what, got, ref):
    """the bounds of the issue: recon and recons 2e-4 of max |reference|; masks 1e-4 max |logit| (first order: |d softmax| <= max |d z| / 2
    with the logits held to 2e-4 of their maximum), and sums to 1 within 1e-5"""
    recon, recons, masks = got
    e_recon, e_recons = rel(recon, ref['recon']), rel(recons, ref['recons'])
    e_masks = (masks.cpu().double() - ref['masks']).abs().max().item()
    bound = 1e-4 * ref['logits'].abs().max().item()
    e_sum = (masks.sum(1) - 1.).abs().max().item()
    print(f'{what}: recon {e_recon:.2e} recons {e_recons:.2e} (bound 2e-4)  masks {e_masks:.2e} (bound {bound:.2e})  |sum - 1| {e_sum:.1e}')
    assert e_recon < 2e-4 and e_recons < 2e-4
    assert e_masks <= bound
    assert e_sum <= 1e-5


def decode_all(m, slots, fg_thre=dc.FG_THRE):
    """one sf_savi_decode_seg_f32 call with all five outputs: recon_combined, recons, masks, seg_i64, seg_u8"""
    from slotformer_amd import engine
    from slotformer_amd._lib import lib, check
    plan = engine.decoder_plan(m)
    F_, N, _ = slots.shape
    H, dev = plan.struct.resolution, slots.device
    recon = torch.full((F_, 3, H, H), float('nan'), device=dev)
    recons = torch.full((F_, N, 3, H, H), float('nan'), device=dev)
    masks = torch.full((F_, N, 1, H, H), float('nan'), device=dev)
    s64 = torch.full((F_, H, H), -1, device=dev, dtype=torch.int64)
    s8 = torch.full((F_, H, H), 255, device=dev, dtype=torch.uint8)
    ws = engine.workspace(dev, lib().sf_savi_decode_workspace_bytes(C.byref(plan.struct), F_), ('dec', 0))
    check(lib().sf_savi_decode_seg_f32(C.byref(plan.struct), slots.data_ptr(), recon.data_ptr(), recons.data_ptr(), masks.data_ptr(),
                                       s64.data_ptr(), s8.data_ptr(), float(fg_thre), F_, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream))
    return recon, recons, masks, s64, s8


# ---- a: every case against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', dc.NAMES)
@torch.no_grad()
def test_decode_vs_float64(dev, precision, name):
    res, N, D, ch, r, ks, F_ = dc.CASES[name]
    m, ref = model(name, dev), dc.reference(name)
    slots = dc.case_slots(name).to(dev)
    recon, recons, masks, s = m.decode(slots)
    assert s is slots
    assert recon.shape == (F_, 3, res, res) and recons.shape == (F_, N, 3, res, res) and masks.shape == (F_, N, 1, res, res)
    check_against_float64(f'decode {name} {precision}', (recon, recons, masks), ref)


# ---- b: the segmentation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seg_dtype', [torch.int64, torch.uint8], ids=['i64', 'u8'])
@pytest.mark.parametrize('name', dc.NAMES)
@torch.no_grad()
def test_segmentation(dev, precision, name, seg_dtype):
    from slotformer_amd import engine
    from slotformer_amd.video_prediction.vp_utils import postproc_mask
    m, ref = model(name, dev), dc.reference(name)
    slots = dc.case_slots(name).to(dev)
    recon, recons, masks, seg = engine.savi_decode(m, slots, want=('recons', 'masks', 'seg'), seg_dtype=seg_dtype)
    assert seg.dtype == seg_dtype and seg.shape == ref['seg'].shape
    seg = seg.cpu().long()
    # the rule on the decoder's own float32 masks: no pixel excepted
    own = oracle.postproc_mask(masks.cpu().unsqueeze(0), dc.FG_THRE)[0]
    assert torch.equal(seg, own)
    assert len(torch.unique(seg)) >= 3 and (seg != masks.cpu().squeeze(2).argmax(1)).any()    # (not the all-background frames of plain weights)
    # the rule on the float64 masks, outside the pixels that sit on one of its decisions
    ok = ~ref['excluded'].view(seg.shape)
    print(f'segmentation {name} {precision}: {(seg != ref["seg"]).sum().item()} pixels differ from float64, {(~ok).sum().item()} excluded of {ok.numel()}')
    assert torch.equal(seg[ok], ref['seg'][ok])
    vp = postproc_mask(masks.unsqueeze(0))[0].cpu()
    assert torch.equal(vp, own) and torch.equal(vp[ok], ref['seg'][ok])


# ---- c: optional outputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', dc.NAMES)
@torch.no_grad()
def test_optional_outputs(dev, precision, name):
    from slotformer_amd import engine
    m = model(name, dev)
    slots = dc.case_slots(name).to(dev)
    for seg_dtype in (torch.int64, torch.uint8):
        recon, recons, masks, seg = engine.savi_decode(m, slots, want=('recons', 'masks', 'seg'), seg_dtype=seg_dtype)
        r0, a, b = engine.savi_decode(m, slots, want=())
        assert a is None and b is None and torch.equal(r0, recon)
        r1, a, b, s1 = engine.savi_decode(m, slots, want=('seg', ), seg_dtype=seg_dtype)
        assert a is None and b is None and torch.equal(r1, recon)
        assert s1.dtype == seg_dtype and torch.equal(s1, seg)
        r2, a, b = engine.savi_decode(m, slots, want=('masks', ))
        assert a is None and torch.equal(r2, recon) and torch.equal(b, masks)


# ---- d: the frame-chunk loop ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_chunk_loop_phyre(dev, precision):
    """33 frames of the PHYRE decoder = a chunk of 32 and a chunk of 1: every output of the second chunk lands behind the first."""
    from slotformer_amd import engine
    from slotformer_amd._lib import lib
    m = model('phyre', dev)
    plan = engine.decoder_plan(m)
    ws = lambda n: lib().sf_savi_decode_workspace_bytes(C.byref(plan.struct), n)   # noqa: E731
    # the workspace grows with the frames of one chunk: it stops growing exactly where the second chunk begins
    assert ws(33) == ws(32) and ws(32) > ws(31)
    slots = dc.case_slots('phyre', F=33).to(dev)
    whole = decode_all(m, slots)
    first, last = decode_all(m, slots[:32].contiguous()), decode_all(m, slots[32:33].contiguous())
    for name, w, a, b in zip(('recon_combined', 'recons', 'masks', 'seg_i64', 'seg_u8'), whole, first, last):
        assert torch.equal(w[:32], a), name
        assert torch.equal(w[32:33], b), name
    assert torch.equal(whole[3], whole[4].long()) and int(whole[3].min()) >= 0 and int(whole[3].max()) < 8
    frames = [0, 31, 32]
    ref = dc.reference('phyre', F=33, frames=(0, 31, 32))
    check_against_float64(f'chunked decode phyre {precision}', tuple(t[frames] for t in whole[:3]), ref)
    seg = whole[3][frames].cpu()
    ok = ~ref['excluded'].view(seg.shape)
    assert torch.equal(seg[ok], ref['seg'][ok])


# ---- e: sf_decode_combine_seg_f32 on crafted head outputs -------------------------------------------------------------------------------
def crafted_dec(F_, N, HW, seed):
    """dec [F, N, HW, 4] float32.  Frame 0, pixel 0: slot 0 at +80, the others at -80; pixel 1: every slot at +80; pixel 2: every slot at -80
    (the maximum has to be subtracted before the exponential); pixel 3: slots 0 and 1 share the top logit (N = 2: both masks are exactly
    0.5).  Last frame (F > 1): slots a < b with the same logits everywhere, 6 below the others' -- two equal lowest peaks, a is the
    background."""
    rs = np.random.RandomState(seed)
    dec = rs.standard_normal((F_, N, HW, 4)).astype(np.float32)
    dec[..., 3] *= 3.
    if N == 2:
        dec[0, :, :, 3] /= 3.     # (so that no mask of frame 0 rounds to 1 but the crafted one: slot 1 is its background)
    dec[0, :, 0, 3] = -80.
    dec[0, 0, 0, 3] = 80.
    dec[0, :, 1, 3] = 80.
    dec[0, :, 2, 3] = -80.
    dec[0, :, 3, 3] = -5.
    dec[0, :2, 3, 3] = 2.
    a, b = (1, N - 1) if N >= 3 else (0, N - 1)
    if N >= 2 and F_ > 1:
        dec[F_ - 1, a, :, 3] -= 6.
        dec[F_ - 1, b, :, 3] = dec[F_ - 1, a, :, 3]
    return dec, a, b


@pytest.mark.parametrize('F_,HW', [(1, 256), (3, 100), (2, 4096)])
@pytest.mark.parametrize('N', [1, 2, 7, 8, 9, 16])
def test_combine_seg_crafted(dev, N, F_, HW):
    from slotformer_amd._lib import lib, check
    dec_np, a, b = crafted_dec(F_, N, HW, seed=N * 10 + F_)
    dec = torch.from_numpy(dec_np)
    z = dec[..., 3].double()                                               # [F, N, HW]
    ref_masks = torch.softmax(z, 1)
    rgb = dec[..., :3].permute(0, 1, 3, 2).contiguous()                    # [F, N, 3, HW]
    ref_recon = (rgb.double() * ref_masks.unsqueeze(2)).sum(1)
    mag = (rgb.double().abs() * ref_masks.unsqueeze(2)).sum(1)
    dd = dec.reshape(F_ * N, HW, 4).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def run(thre, recons, masks, i64, u8):
        recon = torch.full((F_, 3, HW), float('nan'), device=dev)
        rs = torch.full((F_, N, 3, HW), float('nan'), device=dev) if recons else None
        mk = torch.full((F_, N, HW), float('nan'), device=dev) if masks else None
        s64 = torch.full((F_, HW), -1, device=dev, dtype=torch.int64) if i64 else None
        s8 = torch.full((F_, HW), 255, device=dev, dtype=torch.uint8) if u8 else None
        scratch = torch.full((F_ * N, ), 0x7fffffff, device=dev, dtype=torch.int32)
        P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        check(lib().sf_decode_combine_seg_f32(dd.data_ptr(), recon.data_ptr(), P(rs), P(mk), P(s64), P(s8), float(thre), scratch.data_ptr(),
                                              F_, N, HW, st))
        return recon, rs, mk, s64, s8

    for thre in (0.5, 0., 1.01):
        recon, rs, mk, s64, s8 = (None if t is None else t.cpu() for t in run(thre, True, True, True, True))
        # float32 rounding: the subtraction of the maximum (|z - max| < 32 off the +-80 pixels), expf, the sum, the reciprocal and the product
        assert ((mk.double() - ref_masks).abs() <= 1e-5 * ref_masks + 1e-30).all()
        assert ((recon.double() - ref_recon).abs() <= 2e-5 * mag + 1e-30).all()
        assert torch.equal(rs, rgb)
        want = oracle.postproc_mask(mk.view(1, F_, N, 1, HW, 1), thre)[0].view(F_, HW)
        assert torch.equal(s64, want) and torch.equal(s8.long(), want)
        if thre == 0.:
            assert torch.equal(want, mk.argmax(1))
        # the crafted pixels are what they are meant to be in the returned masks
        assert mk[0, 0, 0] == 1. and (mk[0, 1:, 0] == 0.).all()
        assert (mk[0, :, 1] == mk[0, 0, 1]).all() and (mk[0, :, 2] == mk[0, 0, 2]).all() and abs(mk[0, 0, 1].item() * N - 1.) < 1e-6
        if N >= 2:
            assert mk[0, 0, 3] == mk[0, 1, 3] and (mk[0, 2:, 3] < mk[0, 0, 3]).all()
            if thre == 0.:
                assert want[0, 3] == 0                                    # equal top logits: the lower index
        if N >= 2 and F_ > 1:
            peaks = mk[F_ - 1].max(-1)[0]
            assert peaks[a] == peaks[b] and (peaks[a] <= peaks).all()
            if thre == 0.5 and N > 2:
                assert ((mk[F_ - 1].max(0)[0] < 0.5) == (want[F_ - 1] == a)).any()        # equal lowest peaks: the lower index is the background
                assert (want[F_ - 1][mk[F_ - 1].max(0)[0] < 0.5] == a).all()
        if N == 2 and thre == 0.5:
            # exactly 0.5 is not below the threshold: the pixel keeps its argmax (slot 0), though slot 1 is this frame's background
            assert mk[0, 0, 3] == 0.5 and mk[0, 0].max() > mk[0, 1].max() and want[0, 3] == 0
        # outputs left out: the same bits in the others
        r2, _, _, _, u2 = run(thre, False, False, False, True)
        assert torch.equal(r2.cpu(), recon) and torch.equal(u2.cpu(), s8)
        r3, _, m3, i3, _ = run(thre, False, True, True, False)
        assert torch.equal(r3.cpu(), recon) and torch.equal(m3.cpu(), mk) and torch.equal(i3.cpu(), s64)
        r4, q4, _, _, _ = run(thre, True, False, False, False)
        assert torch.equal(r4.cpu(), recon) and torch.equal(q4.cpu(), rs)


# ---- f: sf_postproc_mask_f32 on arbitrary floats ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('HW', [100, 4096])
@pytest.mark.parametrize('N', [1, 7, 17, 255])
def test_postproc_mask_any_float(dev, N, HW):
    """Frames 0, 1: standard-normal values (at N = 1 half of the pixels have a negative best value).  Frame 2: every value negative, so every
    slot peak takes the negative branch of the key, every pixel is below the threshold and goes to the slot with the most negative peak.  Frame 3: slot a peaks at +0.0, a later slot b at
    -0.0, every other slot above: torch.argmin takes them as equal, the first is the background."""
    from slotformer_amd._lib import lib, check
    from slotformer_amd.video_prediction.vp_utils import postproc_mask
    rs = np.random.RandomState(N + HW)
    mk = rs.standard_normal((4, N, HW)).astype(np.float32)
    mk[2:] = -np.abs(mk[2:]) - np.float32(0.1)
    a, b = (1, N - 1) if N >= 3 else (0, N - 1)
    mk[3, :, 7] = 1. + np.arange(N, dtype=np.float32) / N                # (pixel 7: above the threshold in every slot but a and b)
    mk[3, a, 7] = mk[3, a, 8]
    mk[3, b, 7] = mk[3, b, 8]
    mk[3, a, 11] = 0.
    mk[3, b, 13] = -0.
    masks = torch.from_numpy(mk)
    if N >= 2:
        peaks = masks[3].max(-1)[0]
        assert peaks[a] == 0 and peaks[b] == 0 and not np.signbit(peaks[a].item()) and np.signbit(peaks[b].item())
        assert sorted(peaks.tolist())[2 if N > 2 else 1] >= (1. if N > 2 else 0.)
    want = oracle.postproc_mask(masks.view(1, 4, N, 1, HW, 1), dc.FG_THRE)[0].view(4, HW)
    assert (want[2] == masks[2].max(-1)[0].argmin()).all()
    if N >= 2:
        assert (want[3] == a).sum() >= HW - 3 and not (want[3] == b).any()
    md = masks.to(dev)
    s64 = torch.full((4, HW), -1, device=dev, dtype=torch.int64)
    s8 = torch.full((4, HW), 255, device=dev, dtype=torch.uint8)
    scratch = torch.zeros(4 * N, device=dev, dtype=torch.int32)
    check(lib().sf_postproc_mask_f32(md.data_ptr(), s64.data_ptr(), s8.data_ptr(), dc.FG_THRE, scratch.data_ptr(), 4, N, HW,
                                     torch.cuda.current_stream().cuda_stream))
    for f in range(4):
        assert torch.equal(s64[f].cpu(), want[f]), f'frame {f}'
    assert torch.equal(s8.cpu().long(), want)
    assert torch.equal(postproc_mask(md.view(1, 4, N, 1, HW, 1)).cpu().view(4, HW), want)


# ---- g: the fragment deconvolution off the square --------------------------------------------------------------------------------------
def _deconv_inputs(R, H, W, seed):
    """x [R,H,W,64] with image 0 zero but for its four corner pixels (a halo or border slip shows as a whole wrong value), weight, bias"""
    rs = np.random.RandomState(seed)
    t = lambda *s, scale=1.: torch.from_numpy((rs.standard_normal(s) * scale).astype(np.float32))   # noqa: E731
    x = t(R, H, W, 64)
    corners = x[0, [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]].clone()
    x[0] = 0.
    x[0, [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = corners
    return x, t(64, 64, 5, 5, scale=(64 * 6.25)**-0.5), t(64, scale=0.1), rs


def _refused_in_f32(fn):
    with pytest.raises(RuntimeError, match='split-bf16 mode only'):
        fn()


@pytest.mark.parametrize('R,H,W', [(1, 4, 64), (2, 8, 32), (2, 48, 16), (3, 12, 64)])
def test_deconv_frag_off_square(dev, precision, R, H, W):
    from slotformer_amd import ops
    x, w, b, _ = _deconv_inputs(R, H, W, seed=H * 100 + W + R)
    frag = ops.pack_deconv_frag(ops.pack_deconv_weight(w.to(dev)))
    if precision == 'f32':        # the fragments are split-bf16: the entry point refuses, it does not compute something else
        return _refused_in_f32(lambda: ops.deconv5x5s2_frag(x.to(dev), frag, b.to(dev)))
    ref = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=2, output_padding=1).permute(0, 2, 3, 1)
    out = ops.deconv5x5s2_frag(x.to(dev), frag, b.to(dev), relu=False)
    assert out.shape == (R, 2 * H, 2 * W, 64)
    r1 = close(out, ref, TOL['bf16x3'], 'deconv')
    r2 = close(ops.deconv5x5s2_frag(x.to(dev), frag, b.to(dev), relu=True), F.relu(ref), TOL['bf16x3'], 'deconv + relu')
    print(f'deconv frag R {R} H {H} W {W}: error / bound {r1:.3f} (plain) {r2:.3f} (relu)')


@pytest.mark.parametrize('R,H', [(1, 4), (2, 8)])
def test_deconv_head_frag_off_square(dev, precision, R, H):
    from slotformer_amd import ops
    W = 64
    x, w, b, rs = _deconv_inputs(R, H, W, seed=H * 7 + R)
    hw = torch.from_numpy((rs.standard_normal((4, 64)) * 0.2).astype(np.float32))
    hb = torch.from_numpy((rs.standard_normal(4) * 0.1).astype(np.float32))
    frag = ops.pack_deconv_frag(ops.pack_deconv_weight(w.to(dev)))
    if precision == 'f32':
        return _refused_in_f32(lambda: ops.deconv5x5s2_head(x.to(dev), frag, b.to(dev), hw.to(dev), hb.to(dev)))
    y = F.relu(F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=2, output_padding=1))
    ref = F.conv2d(y, hw.double().view(4, 64, 1, 1), hb.double()).permute(0, 2, 3, 1).reshape(R, 4 * H * W, 4)
    dec = ops.deconv5x5s2_head(x.to(dev), frag, b.to(dev), hw.to(dev), hb.to(dev))
    assert dec.shape == ref.shape
    r = close(dec, ref, TOL['bf16x3'], 'deconv + head')
    print(f'deconv head frag R {R} H {H}: error / bound {r:.3f}')
