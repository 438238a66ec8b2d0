"""CPU: the plain-torch home of slotformer_amd.egress and the reference's names in video_prediction/vp_vis.py against checkers written here,
independent of the implementation: a loop-per-tile numpy make_grid from torchvision's rule, PIL.ImageDraw for outlines and a loop-per-pixel form of
the stated outline rule (tests/egress_cases.py).  Everything is integer-valued or a fixed sequence of float32 operations, so it is held to EXACT
equality.  The device kernels are held to this home in tests/test_egress_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

import egress_cases as ec


def _eq(got, ref):
    got = got.numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), f'{int((got != ref).sum())} of {ref.size} differ'


@pytest.mark.parametrize('H,W', ec.SIZES)
@pytest.mark.parametrize('K', [1, 2, 5])
def test_video_grid_is_make_grid(H, W, K):
    from slotformer_amd import egress
    for scale in (1., 0.):
        inputs = ec.grid_inputs(H, W)
        for nrow, padding, pad_value in itertools.product(sorted({1, K, 2}), (0, 2), (0., 1.)):
            ref = ec.np_grid_video(K, inputs, scale, nrow, padding, pad_value)
            tiles = ec.torch_tiles(K, *inputs, scale)
            _eq(egress.video_grid(tiles, nrow=nrow, padding=padding, pad_value=pad_value), ref)
            _eq(egress.video_grid(tiles, nrow=nrow, padding=padding, pad_value=pad_value, dtype=torch.uint8), ec.np_u8(ref))
            _eq(egress.video_grid(tiles, nrow=nrow, padding=padding, pad_value=pad_value, dtype=torch.uint8, layout='hwc'),
                np.ascontiguousarray(ec.np_u8(ref).transpose(0, 2, 3, 1)))
        # nrow=None: one row
        _eq(egress.video_grid(ec.torch_tiles(K, *inputs, scale)), ec.np_grid_video(K, inputs, scale, K, 2, 0.))
    # uint8 ids give the same picture as int64 ids
    if K > 1:
        inputs = ec.grid_inputs(H, W)
        assert torch.equal(egress.video_grid(ec.torch_tiles(K, *inputs, 1., ids_dtype=torch.uint8)), egress.video_grid(ec.torch_tiles(K, *inputs, 1.)))


@pytest.mark.parametrize('H,W', ec.SIZES)
@pytest.mark.parametrize('K', [1, 2, 5])
def test_video_grid_borders(H, W, K):
    from slotformer_amd import egress
    inputs = ec.grid_inputs(H, W, seed=1)
    for hists in ((0, 0, 0), (2, 2, 2), (ec.T, ec.T, ec.T), (ec.T, 2, 0)):
        for width, nrow, padding in ((2, 1, 0), (1, 2, 2), (3, K, 2)):
            border = (width, hists)
            ref = ec.np_grid_video(K, inputs, 1., nrow, padding, 1., border)
            tiles = ec.torch_tiles(K, *inputs, 1., border=border)
            _eq(egress.video_grid(tiles, nrow=nrow, padding=padding, pad_value=1.), ref)
            _eq(egress.video_grid(tiles, nrow=nrow, padding=padding, pad_value=1., dtype=torch.uint8), ec.np_u8(ref))
    assert int(ec.np_u8(np.full((1, ), 0.7, dtype=np.float32))[0]) == 178     # 0.7f * 255.f = 178.49998: the cast truncates


@pytest.mark.parametrize('H,W', ec.SIZES)
def test_make_video_and_slot_decomposition_grid(H, W):
    """the reference's lines (vp_vis.py:29-50, base_slots/method.py:102-131) re-expressed with the numpy checker"""
    from slotformer_amd.video_prediction import vp_vis
    img, recons, masks, _, _ = ec.grid_inputs(H, W, seed=2)
    pred = ec.grid_inputs(H, W, seed=3)[0]
    T, N = ec.T, ec.N
    for hist in (0, 2, T):
        a, b = ec.np_to_rgb(img), ec.np_to_rgb(pred)
        ref = np.stack([ec.np_make_grid(np.stack([ec.np_add_boundary(a[t], 2, True), ec.np_add_boundary(b[t], 2, t < hist)]), 1, 0, 0.)
                        for t in range(T)])
        got = vp_vis.make_video(torch.from_numpy(img), torch.from_numpy(pred), hist)
        assert tuple(got.shape) == (T, 3, 2 * (H + 4), W + 4) and got.device.type == 'cpu'
        _eq(got, ref)
        _eq(vp_vis.make_video_u8(torch.from_numpy(img), torch.from_numpy(pred), hist), np.ascontiguousarray(ec.np_u8(ref).transpose(0, 2, 3, 1)))
    # a non-contiguous input, as test_vp.py:181 hands over (palette lookup permuted to CHW)
    nc = torch.from_numpy(img).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nc.is_contiguous() and torch.equal(vp_vis.make_video(nc, nc, 2), vp_vis.make_video(torch.from_numpy(img), torch.from_numpy(img), 2))
    for scale in (1., 0.):
        out = ec.np_to_rgb(np.concatenate([img[:, None], pred[:, None], recons * masks + (np.float32(1.) - masks) * np.float32(scale)], 1))
        ref = np.stack([ec.np_make_grid(out[t], N + 2, 2, np.float32(1. - scale)) for t in range(T)])
        args = [torch.from_numpy(x) for x in (img, pred, recons, masks)]
        got = vp_vis.slot_decomposition_grid(*args, scale=scale)
        assert tuple(got.shape) == (T, 3, H + 4, (N + 2) * (W + 2) + 2)
        _eq(got, ref)
        _eq(vp_vis.slot_decomposition_grid(*args, scale=scale, dtype=torch.uint8), ec.np_u8(ref))
    # add_boundary
    x = torch.rand(2, 3, H, W)
    for colour in ('red', 'green'):
        _eq(vp_vis.add_boundary(x, 2, colour), np.stack([ec.np_add_boundary(x[t].numpy(), 2, colour == 'green') for t in range(2)]))


def test_frames_to_uint8_both_roundings():
    from slotformer_amd import egress
    k = np.arange(256, dtype=np.float32)
    x = np.float32(2.) * k / np.float32(255.) - np.float32(1.)
    vals = np.concatenate([x, np.nextafter(x, np.float32(-2)), np.nextafter(x, np.float32(2)), np.array([-1.5, 1.5, 0., -0.], dtype=np.float32)])
    n = 3 * 13 * 7
    frames = np.resize(vals, 5 * n).reshape(5, 3, 13, 7)
    v = np.clip(frames * np.float32(0.5) + np.float32(0.5), 0, 1) * np.float32(255.)
    t = torch.from_numpy(frames)
    _eq(egress.frames_to_uint8(t, layout='chw'), v.astype(np.uint8))
    _eq(egress.frames_to_uint8(t, layout='chw', rounding='nearest'), np.rint(v).astype(np.uint8))
    _eq(egress.frames_to_uint8(t), np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 1)))
    # without to_rgb: [0, 1] values, anything outside clamped so that nothing wraps
    raw = np.array([-0.3, 0., 0.5, 0.7, 1., 1.01, 2.], dtype=np.float32)
    fr = np.resize(raw, n).reshape(1, 3, 13, 7)
    _eq(egress.frames_to_uint8(torch.from_numpy(fr), to_rgb=False, layout='chw'), np.clip(fr * np.float32(255.), 0, 255).astype(np.uint8))
    # leading dimensions and out=
    out = torch.zeros(1, 5, 13, 7, 3, dtype=torch.uint8)
    assert egress.frames_to_uint8(t[None], out=out) is out and torch.equal(out[0], egress.frames_to_uint8(t))


def test_boxes_against_pil():
    """width 2, M = 4, 24 x 20, both sides of every box >= 4: the colour is the rank among the KEPT boxes and later boxes overwrite earlier ones"""
    from slotformer_amd import egress
    from slotformer_amd.video_prediction.vp_utils import PALETTE_np
    frames, boxes, pres = ec.box_case()
    ref = ec.pil_boxes(frames, boxes, pres, PALETTE_np, ec.BOX_WIDTH)
    assert np.array_equal(ref, ec.rule_boxes(frames, boxes, pres, PALETTE_np, ec.BOX_WIDTH))    # (the rule is PIL's here)
    assert (ref != frames).any(axis=1).sum() > 200
    got = torch.from_numpy(frames.copy())
    assert egress.draw_boxes_(got, torch.from_numpy(boxes), torch.from_numpy(pres), width=ec.BOX_WIDTH) is got
    _eq(got, ref)
    # a bool mask and an explicit palette do the same; without the mask frame 1 gains a box and every later colour moves on by one
    got2 = egress.draw_boxes_(torch.from_numpy(frames.copy()), torch.from_numpy(boxes), torch.from_numpy(pres).bool(), palette=PALETTE_np, width=2)
    _eq(got2, ref)
    _eq(egress.draw_boxes_(torch.from_numpy(frames.copy()), torch.from_numpy(boxes)), ec.pil_boxes(frames, boxes, None, PALETTE_np, 2))
    # the reference's entry: round to uint8, draw, back to [-1, 1]
    from slotformer_amd.video_prediction import vp_vis
    imgs = torch.from_numpy(frames).float() / 255. * 2. - 1.
    back = vp_vis.batch_draw_bbox(imgs, torch.from_numpy(boxes), torch.from_numpy(pres))
    assert back.dtype == torch.float32 and torch.equal(back, torch.from_numpy(ref).float() / 255. * 2. - 1.)
    one = vp_vis.draw_bbox(imgs[0], torch.from_numpy(boxes[0]))
    assert torch.equal(one, back[0])


def test_thin_boxes_follow_the_stated_rule():
    """sides 1 .. 3 < 2 * width: inside the inclusive box only (PIL paints outside such a box: the one documented difference)"""
    from slotformer_amd import egress
    from slotformer_amd.video_prediction.vp_utils import PALETTE_np
    frames, boxes = ec.thin_box_case()
    for width in (2, 1, 3):
        got = egress.draw_boxes_(torch.from_numpy(frames.copy()), torch.from_numpy(boxes), width=width)
        _eq(got, ec.rule_boxes(frames, boxes, None, PALETTE_np, width))


def test_error_paths():
    from slotformer_amd import egress
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match='float32'):
        egress.frames_to_uint8(x.double())
    with pytest.raises(ValueError, match='contiguous'):
        egress.frames_to_uint8(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match=r'\[\.\.\., 3, H, W\]'):
        egress.frames_to_uint8(torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError, match='out must be'):
        egress.frames_to_uint8(x, out=torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match='rounding'):
        egress.frames_to_uint8(x, rounding='up')
    with pytest.raises(ValueError, match='float32'):
        egress.Img(x.half())
    with pytest.raises(ValueError, match='contiguous'):
        egress.Img(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match='uint8 or int64'):
        egress.Ids(torch.zeros(2, 8, 8, dtype=torch.int32))
    for bad in (torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 3), torch.zeros(3, dtype=torch.uint8), torch.zeros(0, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r'\[P, 3\] uint8'):
            egress.Ids(torch.zeros(2, 8, 8, dtype=torch.uint8), bad)
        with pytest.raises(ValueError, match=r'\[P, 3\] uint8'):
            egress.draw_boxes_(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 1, 4), palette=bad)
    with pytest.raises(ValueError, match='masks'):
        egress.Slots(torch.zeros(2, 3, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match='share T, H, W'):
        egress.video_grid([egress.Img(x), egress.Img(torch.zeros(2, 3, 8, 9))])
    with pytest.raises(ValueError, match='border'):
        egress.video_grid([egress.Img(x, border=(2, 1)), egress.Img(x)])
    with pytest.raises(ValueError, match='float32'):
        egress.video_grid([egress.Img(x)], dtype=torch.float16)
    with pytest.raises(ValueError, match='uint8'):
        egress.draw_boxes_(x, torch.zeros(2, 1, 4))
    with pytest.raises(ValueError, match='float32'):
        egress.draw_boxes_(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 1, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match='contiguous'):
        egress.draw_boxes_(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, 2).permute(0, 2, 1))
