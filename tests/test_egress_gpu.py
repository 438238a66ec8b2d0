"""GPU: the egress kernels (csrc/egress.hip) against the plain-torch home of slotformer_amd.egress on the same inputs -- EXACT equality: the results
are bytes, or float32 values of a fixed sequence of float32 operations, and the inputs sit on the truncation boundaries (a product contracted into
an fma would land on the other side) -- and the 'recon_u8' path of the pipeline / the harness against egress.frames_to_uint8 of what today's
device path returns."""
import numpy as np
import pytest
import torch

import egress_cases as ec
import golden_util as gu

pytestmark = pytest.mark.gpu


def _boundary_values():
    x = torch.arange(256, dtype=torch.float32) * 2. / 255. - 1.      # 2k / 255 - 1
    return torch.cat([x, torch.nextafter(x, torch.tensor(-2.)), torch.nextafter(x, torch.tensor(2.)), torch.tensor([-1.5, 1.5, 0., -0.])])


@pytest.mark.parametrize('H,W', [(13, 7), (8, 16)])
def test_frames_to_uint8(dev, H, W):
    from slotformer_amd import egress
    F = 5
    n = F * 3 * H * W
    vals = _boundary_values()
    x = vals.repeat(-(-n // vals.numel()))[:n].reshape(F, 3, H, W).contiguous()
    assert n >= vals.numel()
    for to_rgb in (True, False):
        src = x if to_rgb else (x * 0.6 + 0.5).contiguous()             # ([-0.4, 1.4]: both clamps at work)
        for rounding in ('trunc', 'nearest'):
            for layout in ('chw', 'hwc'):
                ref = egress.frames_to_uint8(src, to_rgb=to_rgb, layout=layout, rounding=rounding)
                for off_in in (0, 4, 12):
                    big = torch.zeros(n + 8, device=dev)
                    xin = big[off_in // 4:off_in // 4 + n].view(F, 3, H, W)
                    xin.copy_(src)
                    assert xin.data_ptr() % 16 == off_in
                    for off_out in (0, 4, 12):
                        obuf = torch.full((n + 32, ), 77, dtype=torch.uint8, device=dev)
                        out = obuf[off_out:off_out + n].view(ref.shape)
                        assert out.data_ptr() % 16 == off_out
                        assert egress.frames_to_uint8(xin, to_rgb=to_rgb, layout=layout, rounding=rounding, out=out) is out
                        assert torch.equal(out.cpu(), ref), (to_rgb, rounding, layout, off_in, off_out)
                        assert bool((obuf[:off_out] == 77).all()) and bool((obuf[off_out + n:] == 77).all())    # nothing beside the span
    assert torch.equal(egress.frames_to_uint8(x.to(dev)).cpu(), egress.frames_to_uint8(x))


@pytest.mark.parametrize('H,W', ec.SIZES)
def test_video_grid(dev, H, W):
    """all three tile kinds at once (K = 5), softmax masks over random-mantissa recons, an id >= P, the border colour changing at history_len = 2"""
    from slotformer_amd import egress
    for scale in (1., 0.):
        inputs = ec.grid_inputs(H, W, seed=4)
        for border in (None, (2, (ec.T, 2, 2))):
            for nrow, padding, pad_value in ((5, 2, 1. - scale), (2, 2, 0.), (1, 0, 1.)):
                for dtype, layout in ((torch.float32, 'chw'), (torch.uint8, 'chw'), (torch.uint8, 'hwc')):
                    kw = dict(nrow=nrow, padding=padding, pad_value=pad_value, dtype=dtype, layout=layout)
                    ref = egress.video_grid(ec.torch_tiles(5, *inputs, scale, border=border), **kw)
                    for ids_dtype in (torch.int64, torch.uint8):
                        got = egress.video_grid(ec.torch_tiles(5, *inputs, scale, border=border, device=dev, ids_dtype=ids_dtype), **kw)
                        assert got.is_cuda and got.dtype == dtype and torch.equal(got.cpu(), ref), (scale, border, nrow, padding, dtype, layout)
    # one tile: handed back as it is; and the reference's names on device tensors
    from slotformer_amd.video_prediction import vp_vis
    img, recons, masks, _, _ = [torch.from_numpy(a) for a in ec.grid_inputs(H, W, seed=5)]
    assert torch.equal(egress.video_grid([egress.Img(img.to(dev))]).cpu(), egress.video_grid([egress.Img(img)]))
    got = vp_vis.make_video(img.to(dev), img.flip(0).contiguous().to(dev), 2)
    assert got.device.type == 'cpu' and torch.equal(got, vp_vis.make_video(img, img.flip(0).contiguous(), 2))
    got = vp_vis.make_video_u8(img.to(dev), img.flip(0).contiguous().to(dev), 2)
    assert got.is_cuda and torch.equal(got.cpu(), vp_vis.make_video_u8(img, img.flip(0).contiguous(), 2))
    args = (img, img.flip(0).contiguous(), recons, masks)
    for dtype in (torch.float32, torch.uint8):
        got = vp_vis.slot_decomposition_grid(*[a.to(dev) for a in args], scale=0., dtype=dtype)
        assert torch.equal(got.cpu(), vp_vis.slot_decomposition_grid(*args, scale=0., dtype=dtype))


def test_video_grid_vector_path(dev):
    """W % 4 == 0 and aligned sources take the 16-byte loads; a source at a 4-byte offset takes the scalar path: the same bits"""
    from slotformer_amd import egress
    H, W = 6, 16
    inputs = ec.grid_inputs(H, W, seed=6)
    kw = dict(nrow=3, padding=2, pad_value=0.5, dtype=torch.uint8, layout='hwc')
    ref = egress.video_grid(ec.torch_tiles(5, *inputs, 1., border=(2, (1, 2, 3))), **kw)
    tiles = ec.torch_tiles(5, *inputs, 1., border=(2, (1, 2, 3)), device=dev)
    assert all(t.data_ptr() % 16 == 0 for tl in tiles for t in tl.tensors())
    assert torch.equal(egress.video_grid(tiles, **kw).cpu(), ref)
    big = torch.zeros(inputs[0].size + 4, device=dev)
    view = big[1:1 + inputs[0].size].view(inputs[0].shape)
    view.copy_(torch.from_numpy(inputs[0]))
    tiles[0] = egress.Img(view, border=(2, 1))
    assert view.data_ptr() % 16 == 4 and torch.equal(egress.video_grid(tiles, **kw).cpu(), ref)


def test_draw_boxes(dev):
    from slotformer_amd import egress
    from slotformer_amd.video_prediction import vp_vis
    frames, boxes, pres = ec.box_case()
    thin_frames, thin_boxes = ec.thin_box_case()
    # + a frame with no surviving box (one padded, the others absent): it must come back untouched
    frames = np.concatenate([frames, thin_frames, frames[:1]])
    boxes = np.concatenate([boxes, thin_boxes, np.array([[[-1, -1, -1, -1], [2, 2, 9, 9], [-1, 0, 5, 5], [3, 3, 12, 12]]], dtype=np.float32)])
    pres = np.concatenate([pres, np.ones((2, 4), dtype=np.uint8), np.array([[1, 0, 1, 0]], dtype=np.uint8)])
    fr, bx, pm = torch.from_numpy(frames), torch.from_numpy(boxes), torch.from_numpy(pres)
    for width in (2, 1):
        ref = egress.draw_boxes_(fr.clone(), bx, pm, width=width)
        got = egress.draw_boxes_(fr.clone().to(dev), bx.to(dev), pm.to(dev), width=width)
        assert torch.equal(got.cpu(), ref)
        assert torch.equal(got[-1].cpu(), fr[-1])
    assert torch.equal(egress.draw_boxes_(fr.clone().to(dev), bx.to(dev)).cpu(), egress.draw_boxes_(fr.clone(), bx))
    # W % 16 == 0 takes 16 pixels per lane; the same frames at a 1-byte offset take one: the same bytes
    rs = np.random.RandomState(7)
    wide = torch.from_numpy(rs.randint(0, 256, size=(5, 3, 24, 32)).astype(np.uint8))
    bw = bx.clone()
    bw[..., 0::2] *= 1.5
    ref = egress.draw_boxes_(wide.clone(), bw, pm)
    assert torch.equal(egress.draw_boxes_(wide.clone().to(dev), bw.to(dev), pm.to(dev)).cpu(), ref)
    big = torch.zeros(wide.numel() + 16, dtype=torch.uint8, device=dev)
    view = big[1:1 + wide.numel()].view(wide.shape)
    view.copy_(wide)
    assert torch.equal(egress.draw_boxes_(view, bw.to(dev), pm.to(dev)).cpu(), ref) and int(big[0]) == 0 and int(big[-15:].sum()) == 0
    # the reference's entry point on device tensors: one download
    imgs = fr.float() / 255. * 2. - 1.
    got = vp_vis.batch_draw_bbox(imgs.to(dev), bx.to(dev), pm.to(dev))
    assert got.device.type == 'cpu' and torch.equal(got, vp_vis.batch_draw_bbox(imgs, bx, pm))


# ---- pipeline / harness --------------------------------------------------------------------------------------------------------------------
def _res64_models(dev):
    from slotformer_amd.base_slots import build_model
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(21)
    savi = build_model(gu.ParamsView(gu.savi_cfg(64, 7, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'))).eval().to(dev)
    savi.testing = True
    roll = SlotRollouter(**gu.C2_ROLL['rollout_dict']).eval().to(dev)
    return savi, roll


@torch.no_grad()
def test_pipeline_recon_u8_and_harness_to_host(dev):
    """run(decoded={'recon_u8': pinned, 'seg': pinned}) = frames_to_uint8 of the 'recon', and the 'seg', of today's device path, in both schedules and
    twice into the same tensors (the one-batch buffers are reused); extract_and_rollout(decoder=, to_host=True) returns the same in pinned memory,
    ragged tail included, with slots bit-equal to the to_host=False call."""
    from slotformer_amd import egress, harness
    from slotformer_amd.pipeline import EncodeRolloutPipeline
    savi, roll = _res64_models(dev)
    B, T, H, nb, R = 3, 6, 4, 2, 64
    V = B * nb + 1
    rs = np.random.RandomState(31)
    vids = torch.from_numpy((rs.rand(V, T, 3, R, R) * 2 - 1).astype(np.float32)).to(dev)
    noises = torch.from_numpy(rs.standard_normal((V, T, 7, 128)).astype(np.float32)).to(dev)
    imgs = [vids[j * B:(j + 1) * B] for j in range(nb)]
    nz = [noises[j * B:(j + 1) * B] for j in range(nb)]
    try:
        ref_slots, ref = harness.extract_and_rollout(savi, roll, vids, H, batch_size=B, noises=noises, decoder=savi)   # today's device path
        ref_u8 = egress.frames_to_uint8(ref['recon']).cpu()
        ref_seg = ref['seg'].cpu()
        assert tuple(ref_u8.shape) == (V, H, R, R, 3) and ref_u8.float().std() > 1.
        harness.release_pipelines()
        pipe = EncodeRolloutPipeline(savi, roll, B, T, H, decoder=savi)
        try:
            d = {'recon_u8': torch.zeros(nb, B, H, R, R, 3, dtype=torch.uint8).pin_memory(), 'seg': torch.zeros(nb, B, H, R, R, dtype=torch.uint8).pin_memory()}
            for serial in (False, True, False):
                d['recon_u8'].fill_(9)
                d['seg'].fill_(9)
                out = pipe.run(imgs, nz, serial=serial, decoded=d)
                assert 'recon' not in d and torch.equal(out, ref_slots[:nb * B].view(nb, B, T + H, 7, 128))
                assert torch.equal(d['recon_u8'].view(nb * B, H, R, R, 3), ref_u8[:nb * B]), serial
                assert torch.equal(d['seg'].view(nb * B, H, R, R), ref_seg[:nb * B]), serial
            # device-resident uint8 frames beside the float32 ones
            d2 = {'recon_u8': torch.zeros(nb, B, H, R, R, 3, dtype=torch.uint8, device=dev), 'recon': torch.zeros(nb, B, H, 3, R, R, device=dev)}
            pipe.run(imgs, nz, decoded=d2)
            torch.cuda.synchronize()
            assert torch.equal(d2['recon_u8'].cpu().view(nb * B, H, R, R, 3), ref_u8[:nb * B]) and d2['seg'].is_cuda
            assert torch.equal(d2['recon'].view(nb * B, H, 3, R, R), ref['recon'][:nb * B])
            with pytest.raises(RuntimeError, match='recon_u8'):
                pipe.run(imgs, nz, decoded={'recon_u8': torch.zeros(nb, B, H, R, R, 3, dtype=torch.uint8)})      # pageable
        finally:
            pipe.close()
        slots_h, dec = harness.extract_and_rollout(savi, roll, vids, H, batch_size=B, noises=noises, decoder=savi, to_host=True)
        assert not slots_h.is_cuda and slots_h.is_pinned() and torch.equal(slots_h, ref_slots.cpu())
        assert sorted(dec) == ['recon_u8', 'seg'] and all(not v.is_cuda and v.is_pinned() for v in dec.values())
        assert tuple(dec['recon_u8'].shape) == (V, H, R, R, 3) and tuple(dec['seg'].shape) == (V, H, R, R)
        assert torch.equal(dec['recon_u8'], ref_u8) and torch.equal(dec['seg'], ref_seg)
    finally:
        harness.release_pipelines()
