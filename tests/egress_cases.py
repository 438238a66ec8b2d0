"""Inputs and independent checkers shared by tests/test_egress.py (CPU) and tests/test_egress_gpu.py: a loop-per-tile numpy make_grid written from
the rule torchvision.utils.make_grid follows, PIL.ImageDraw for rectangle outlines, and a loop-per-pixel form of the stated outline rule."""
import numpy as np
import torch

T, N = 3, 3
SIZES = [(10, 12), (13, 7)]
F32 = np.float32


# ---- checkers ------------------------------------------------------------------------------------------------------------------------------
def np_to_rgb(x):
    return np.clip(x.astype(F32) * F32(0.5) + F32(0.5), F32(0), F32(1))


def np_make_grid(tiles, nrow, padding, pad_value):
    """tiles [K, 3, h, w] float32 -> the canvas of torchvision.utils.make_grid(tiles, nrow, padding, pad_value=pad_value), tile by tile"""
    K, _, h, w = tiles.shape
    if K == 1:
        return tiles[0].copy()
    xmaps = min(nrow, K)
    ymaps = int(np.ceil(K / xmaps))
    canvas = np.full((3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), pad_value, dtype=F32)
    for k in range(K):
        r, c = k // xmaps, k % xmaps
        y0, x0 = r * (h + padding) + padding, c * (w + padding) + padding
        canvas[:, y0:y0 + h, x0:x0 + w] = tiles[k]
    return canvas


def np_add_boundary(tile, width, green):
    _, h, w = tile.shape
    out = np.zeros((3, h + 2 * width, w + 2 * width), dtype=F32)
    out[1 if green else 0] = F32(0.7)
    out[:, width:width + h, width:width + w] = tile
    return out


def np_u8(canvas):
    return (canvas * F32(255.)).astype(np.uint8)     # (values in [0, 1]: the cast truncates, nothing to clamp)


def grid_inputs(H, W, seed=0, scale=1.):
    """img [T,3,H,W], recons [T,N,3,H,W] (random mantissas, so that recons * masks needs rounding), masks = softmax over the N slots, ids [T,H,W]
    int64 with one id >= P, and a palette of P = 5 colours"""
    rs = np.random.RandomState(seed + H * 100 + W)
    img = (rs.rand(T, 3, H, W) * 2.4 - 1.2).astype(F32)
    recons = (rs.rand(T, N, 3, H, W) * 2 - 1).astype(F32)
    logits = rs.standard_normal((T, N, 1, H, W)).astype(F32)
    masks = torch.softmax(torch.from_numpy(logits), 1).numpy()
    pal = rs.randint(0, 256, size=(5, 3)).astype(np.uint8)
    ids = rs.randint(0, 5, size=(T, H, W)).astype(np.int64)
    ids[1, H // 2, W // 2] = 9        # >= P: takes the last colour
    ids[0, 0, 0] = 200
    return img, recons, masks, ids, pal


def np_tiles(K, img, recons, masks, ids, pal, scale):
    """the K = 1 / 2 / 5 tiles of frame-major shape [T, K, 3, H, W] in [0, 1]: image; image + ids; image + N slots + ids"""
    P = pal.shape[0]
    col = pal.astype(F32) / F32(255.) * F32(2.) - F32(1.)
    idt = np_to_rgb(col[np.minimum(ids, P - 1)].transpose(0, 3, 1, 2))
    slots = np_to_rgb(recons * masks + (F32(1.) - masks) * F32(scale))
    parts = {1: [np_to_rgb(img)[:, None]], 2: [np_to_rgb(img)[:, None], idt[:, None]], 5: [np_to_rgb(img)[:, None], slots, idt[:, None]]}[K]
    return np.concatenate(parts, 1)


def torch_tiles(K, img, recons, masks, ids, pal, scale, border=None, device='cpu', ids_dtype=torch.int64):
    from slotformer_amd import egress
    t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    b = lambda h: None if border is None else (border[0], h)   # noqa: E731
    hist = border[1] if border is not None else (0, 0, 0)
    im = egress.Img(t(img), border=b(hist[0]))
    if K == 1:
        return [im]
    idt = egress.Ids(t(ids).to(ids_dtype), t(pal), border=b(hist[2]))
    if K == 2:
        return [im, idt]
    return [im, egress.Slots(t(recons), t(masks), scale, border=b(hist[1])), idt]


def np_grid_video(K, inputs, scale, nrow, padding, pad_value, border=None):
    """border: None or (width, (hist of the image, of the slots, of the ids))"""
    tiles = np_tiles(K, *inputs, scale)
    hists = None
    if border is not None:
        hi, hs, hd = border[1]
        hists = {1: [hi], 2: [hi, hd], 5: [hi] + [hs] * N + [hd]}[K]
    frames = []
    for t in range(T):
        tl = tiles[t]
        if border is not None:
            tl = np.stack([np_add_boundary(tl[k], border[0], t < hists[k]) for k in range(K)])
        frames.append(np_make_grid(tl, nrow, padding, F32(pad_value)))
    return np.stack(frames)


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------------
BOX_H, BOX_W, BOX_WIDTH = 24, 20, 2


def box_case():
    """frames [2, 3, 24, 20] uint8, boxes [2, 4, 4], presence [2, 4]: every box has both sides >= 4.  Frame 0: two overlapping boxes around a padded
    one (-1), and one hanging over the top right corner; frame 1: one absent by mask, one hanging over the bottom edge, one with fractional
    coordinates, one of side exactly 4."""
    rs = np.random.RandomState(5)
    frames = rs.randint(0, 256, size=(2, 3, BOX_H, BOX_W)).astype(np.uint8)
    boxes = np.array([[[2, 3, 12, 14], [-1, -1, -1, -1], [8, 8, 18, 20], [13, -3, 25.7, 6.2]],
                      [[1, 1, 8, 8], [3, 16, 9, 30], [5.9, 4.2, 15.5, 12.9], [10, 10, 14, 14]]], dtype=F32)
    pres = np.array([[1, 1, 1, 1], [0, 1, 1, 1]], dtype=np.uint8)
    return frames, boxes, pres


def thin_box_case():
    """boxes with sides 1 .. 3 (thinner than 2 * width), some on the border of the image"""
    rs = np.random.RandomState(6)
    frames = rs.randint(0, 256, size=(2, 3, BOX_H, BOX_W)).astype(np.uint8)
    boxes = np.array([[[2, 2, 3, 5], [6, 3, 9, 4], [0, 10, 2, 13], [17, 20, 20, 23]],
                      [[4, 4, 5, 5], [10, 2, 13, 12], [3, 15, 12, 17], [18, 0, 19, 3]]], dtype=F32)
    return frames, boxes


def kept_boxes(boxes_f, pres_f):
    keep = boxes_f[:, 0] >= 0
    if pres_f is not None:
        keep &= pres_f != 0
    return [[int(v) for v in b] for b in boxes_f[keep]]      # int() truncates toward zero


def pil_boxes(frames, boxes, pres, palette, width):
    from PIL import Image, ImageDraw
    out = []
    for f in range(frames.shape[0]):
        im = Image.fromarray(np.ascontiguousarray(frames[f].transpose(1, 2, 0)))
        draw = ImageDraw.Draw(im)
        for k, b in enumerate(kept_boxes(boxes[f], None if pres is None else pres[f])):
            draw.rectangle(b, outline=tuple(int(c) for c in palette[k]), width=width)
        out.append(np.asarray(im).transpose(2, 0, 1))
    return np.stack(out)


def rule_boxes(frames, boxes, pres, palette, width):
    """the stated rule, pixel by pixel"""
    out = frames.copy()
    _, _, H, W = frames.shape
    for f in range(frames.shape[0]):
        for k, (x0, y0, x1, y1) in enumerate(kept_boxes(boxes[f], None if pres is None else pres[f])):
            for y in range(H):
                for x in range(W):
                    if x0 <= x <= x1 and y0 <= y <= y1 and (x - x0 < width or x1 - x < width or y - y0 < width or y1 - y < width):
                        out[f, :, y, x] = palette[k]
    return out
