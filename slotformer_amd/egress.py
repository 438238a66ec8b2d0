"""The device side of the way out for pictures: float32 frames, slot decompositions, segment ids and boxes -> the uint8 (or [0, 1] float32) videos
a writer takes -- what the reference builds on the host with torchvision's make_grid / draw_bounding_boxes and `(video * 255.).astype(np.uint8)`
(video_prediction/vp_vis.py, base_slots/method.py:102-131,169-179,293-329) -- csrc/egress.hip.  The mirror image of ingest.py.

Same functions, both homes (the vp_utils.py pattern): device tensors go to the kernels on the current stream, CPU tensors take a plain-torch path
that performs the SAME float32 operations in the same order, so the two agree exactly (the kernels contract nothing into an fma that torch rounds
twice).  Inputs are assumed finite.  File writing stays with the caller.
"""
import ctypes as C

import torch

from . import _lib as L
from ._call import ptr, stream

TRUNC, NEAREST_EVEN = 0, 1
_ROUNDING = {'trunc': TRUNC, 'nearest': NEAREST_EVEN, 'nearest_even': NEAREST_EVEN}
_GRID_MODE = {(torch.float32, 'chw'): 0, (torch.uint8, 'chw'): 1, (torch.uint8, 'hwc'): 2}
IMG, SLOTS, IDS = 0, 1, 2
MAX_TILES = 32
MAX_BOXES = 256
GREEN, RED = (0., 0.7, 0.), (0.7, 0., 0.)

_PALETTES = {}   # device -> the default palette there


def default_palette(device='cpu'):
    """vp_utils.PALETTE_np as a [16, 3] uint8 tensor on `device` (uploaded once per device)."""
    device = torch.device(device)
    key = (device.type, device.index if device.type != 'cuda' or device.index is not None else torch.cuda.current_device())
    if key not in _PALETTES:
        from .video_prediction.vp_utils import PALETTE_np
        _PALETTES[key] = torch.from_numpy(PALETTE_np.copy()).to(device)
    return _PALETTES[key]


def _palette(palette, device):
    if palette is None:
        return default_palette(device)
    pal = torch.as_tensor(palette)
    if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise ValueError(f'slotformer_amd.egress: the palette is a [P, 3] uint8 table with 1 <= P <= 256, got {tuple(pal.shape)} {pal.dtype}')
    return pal.to(device).contiguous()


def _check(x, name, dtypes, shape_doc, ok_shape):
    if not torch.is_tensor(x):
        raise ValueError(f'slotformer_amd.egress: {name} must be a torch tensor, got {type(x).__name__}')
    if x.dtype not in dtypes:
        raise ValueError(f'slotformer_amd.egress: {name} must be {" or ".join(str(d).replace("torch.", "") for d in dtypes)}, got {x.dtype} {tuple(x.shape)}')
    if not ok_shape:
        raise ValueError(f'slotformer_amd.egress: {name} is {shape_doc}, got {tuple(x.shape)}')
    if not x.is_contiguous():
        raise ValueError(f'slotformer_amd.egress: {name} must be contiguous, got shape {tuple(x.shape)} with strides {tuple(x.stride())}')


def to_rgb(x):
    """[-1, 1] -> [0, 1]: clamp(x * 0.5 + 0.5, 0, 1) (to_rgb_from_tensor)"""
    return (x * 0.5 + 0.5).clamp(0, 1)


# ---- (a) frames ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def frames_to_uint8(x, to_rgb=True, layout='hwc', rounding='trunc', out=None):
    """float32 [..., 3, H, W] -> uint8 [..., H, W, 3] (layout 'hwc', what a video writer takes) or [..., 3, H, W] ('chw').
    to_rgb=True: x is in [-1, 1] and v = clamp(x * 0.5 + 0.5, 0, 1); False: v = x, already in [0, 1].  The bytes are rounding(clamp(v * 255., 0, 255)):
    'trunc' casts toward zero as `(video * 255.).numpy().astype(np.uint8)` does (_save_video), 'nearest' is torch.round (draw_bbox).
    Device tensors: one kernel launch on the current stream.  out=: written and returned (it may be a view at any byte offset)."""
    _check(x, 'frames', (torch.float32, ), '[..., 3, H, W]', x.dim() >= 3 and x.shape[-3] == 3 and x.shape[-1] >= 1 and x.shape[-2] >= 1)
    if layout not in ('hwc', 'chw') or rounding not in _ROUNDING:
        raise ValueError(f"slotformer_amd.egress: layout is 'hwc' or 'chw', rounding 'trunc' or 'nearest', got {layout!r} / {rounding!r}")
    lead, (H, W) = tuple(x.shape[:-3]), x.shape[-2:]
    oshape = lead + ((H, W, 3) if layout == 'hwc' else (3, H, W))
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=x.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != oshape or out.dtype != torch.uint8 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f'slotformer_amd.egress: out must be a contiguous uint8 tensor {oshape} on {x.device}, got '
                         f'{tuple(out.shape)} {out.dtype} on {out.device}')
    F = x.numel() // (3 * H * W)
    if F == 0:
        return out
    if x.is_cuda:
        L.check(L.lib().sf_egress_frames_u8(x.data_ptr(), out.data_ptr(), F, H, W, int(layout == 'hwc'), int(bool(to_rgb)), _ROUNDING[rounding],
                                            stream(x)))
        return out
    v = (x * 0.5 + 0.5).clamp(0, 1) if to_rgb else x
    s = (v * 255.).clamp(0, 255)
    if _ROUNDING[rounding] == NEAREST_EVEN:
        s = torch.round(s)
    s = s.to(torch.uint8)
    out.copy_(s.movedim(-3, -1) if layout == 'hwc' else s)
    return out


# ---- (b) grids -------------------------------------------------------------------------------------------------------------------------------
class _Tile:
    border = None

    def _set_border(self, border):
        if border is not None:
            width, hist = border
            if int(width) < 1:
                raise ValueError(f'slotformer_amd.egress: a border is (width >= 1, history_len), got {border!r}')
            self.border = (int(width), int(hist))


class Img(_Tile):
    """one tile per frame: x [T, 3, H, W] float32 in [-1, 1], shown as to_rgb(x).  border=(width, history_len): a frame of `width` pixels around the
    tile, green (0, 0.7, 0) for the frames before `history_len`, red (0.7, 0, 0) from it on (vp_vis.add_boundary)."""
    kind, count = IMG, 1

    def __init__(self, x, border=None):
        _check(x, 'an Img tile', (torch.float32, ), '[T, 3, H, W]', x.dim() == 4 and x.shape[1] == 3)
        self.x = x
        self.T, self.H, self.W, self.device = x.shape[0], x.shape[2], x.shape[3], x.device
        self._set_border(border)

    def tensors(self):
        return (self.x, )

    def entry(self):
        return L.sf_egress_tile(IMG, 1, self.x.data_ptr(), None, 0., 0, 0, 0)

    def rgb(self):
        return to_rgb(self.x)[:, None]


class Slots(_Tile):
    """N tiles per frame: to_rgb(recons * masks + (1 - masks) * scale) with recons [T, N, 3, H, W], masks [T, N, 1, H, W] float32
    (base_slots/method.py:117: scale 1 shows a slot on white, 0 on black)."""
    kind = SLOTS

    def __init__(self, recons, masks, scale=1., border=None):
        _check(recons, 'the recons of a Slots tile', (torch.float32, ), '[T, N, 3, H, W]', recons.dim() == 5 and recons.shape[2] == 3 and recons.shape[1] >= 1)
        T, N, _, H, W = recons.shape
        _check(masks, 'the masks of a Slots tile', (torch.float32, ), f'[{T}, {N}, 1, {H}, {W}]', tuple(masks.shape) == (T, N, 1, H, W))
        if masks.device != recons.device:
            raise ValueError(f'slotformer_amd.egress: recons and masks of a Slots tile live on {recons.device} and {masks.device}')
        self.recons, self.masks, self.scale = recons, masks, float(scale)
        self.T, self.H, self.W, self.device, self.count = T, H, W, recons.device, N
        self._set_border(border)

    def tensors(self):
        return (self.recons, self.masks)

    def entry(self):
        return L.sf_egress_tile(SLOTS, self.count, self.recons.data_ptr(), self.masks.data_ptr(), self.scale, 0, 0, 0)

    def rgb(self):
        return to_rgb(self.recons * self.masks + (1. - self.masks) * self.scale)


class Ids(_Tile):
    """one tile per frame: segment ids [T, H, W], uint8 or int64, coloured through a [P, 3] uint8 palette (default: vp_utils.PALETTE_np) as
    test_vp.py:181-182 does with PALETTE_torch: to_rgb(palette[id] / 255 * 2 - 1).  An id >= P takes colour P - 1."""
    kind, count = IDS, 1

    def __init__(self, seg, palette=None, border=None):
        _check(seg, 'the ids of an Ids tile', (torch.uint8, torch.int64), '[T, H, W]', seg.dim() == 3)
        self.seg, self.palette = seg, _palette(palette, seg.device)
        self.T, self.H, self.W, self.device = seg.shape[0], seg.shape[1], seg.shape[2], seg.device
        self._set_border(border)

    def tensors(self):
        return (self.seg, self.palette)

    def entry(self):
        return L.sf_egress_tile(IDS, 1, self.seg.data_ptr(), self.palette.data_ptr(), 0., int(self.seg.dtype == torch.int64), self.palette.shape[0], 0)

    def rgb(self):
        pal = self.palette.float() / 255. * 2. - 1.
        idx = self.seg.long().clamp(0, self.palette.shape[0] - 1)
        return to_rgb(pal[idx].permute(0, 3, 1, 2))[:, None]


def grid_shape(K, H, W, nrow=None, padding=2, border=0):
    """(CH, CW, xmaps, ymaps, padding) of torchvision.utils.make_grid over K tiles of (H + 2 border) x (W + 2 border); one tile is handed back as
    it is, without padding."""
    TH, TW = H + 2 * border, W + 2 * border
    if K == 1:
        return TH, TW, 1, 1, 0
    xmaps = min(K if nrow is None else int(nrow), K)
    ymaps = -(-K // xmaps)
    return ymaps * (TH + padding) + padding, xmaps * (TW + padding) + padding, xmaps, ymaps, padding


@torch.no_grad()
def video_grid(tiles, nrow=None, padding=2, pad_value=0., dtype=torch.float32, layout='chw'):
    """One video of grids: for every frame t the tiles of `tiles` (a list of Img / Slots / Ids over the same T, H, W; a Slots entry yields N tiles) laid
    out as torchvision.utils.make_grid(tiles_t, nrow, padding, pad_value) lays them (nrow=None: all in one row).  Returns float32 [T, 3, CH, CW] in
    [0, 1] -- what the reference's functions return -- or, with dtype=torch.uint8, the bytes (grid * 255.) cast toward zero as [T, 3, CH, CW]
    (layout 'chw') or [T, CH, CW, 3] ('hwc').  Borders: every tile of a grid has the same size, so either all entries carry border=(width, history_len)
    with one width, or none does; pad_value and the border colours are written as they are.  Device tensors: one kernel launch on the current stream."""
    tiles = list(tiles)
    if not tiles or not all(isinstance(t, _Tile) for t in tiles):
        raise ValueError('slotformer_amd.egress: tiles is a non-empty list of Img / Slots / Ids')
    if (dtype, layout) not in _GRID_MODE:
        raise ValueError(f"slotformer_amd.egress: a grid is float32 'chw', uint8 'chw' or uint8 'hwc', got {dtype} {layout!r}")
    t0 = tiles[0]
    for t in tiles[1:]:
        if (t.T, t.H, t.W) != (t0.T, t0.H, t0.W) or t.device != t0.device:
            raise ValueError(f'slotformer_amd.egress: all tiles of a grid share T, H, W and the device: {(t0.T, t0.H, t0.W)} on {t0.device} '
                             f'and {(t.T, t.H, t.W)} on {t.device}')
    widths = {None if t.border is None else t.border[0] for t in tiles}
    if len(widths) != 1:
        raise ValueError(f'slotformer_amd.egress: the tiles of a grid have one size -- all with a border of one width or none, got {sorted(map(str, widths))}')
    border = widths.pop() or 0
    K = sum(t.count for t in tiles)
    if K > MAX_TILES:
        raise ValueError(f'slotformer_amd.egress: at most {MAX_TILES} tiles per grid, got {K}')
    if int(padding) < 0 or (nrow is not None and int(nrow) < 1):
        raise ValueError(f'slotformer_amd.egress: padding >= 0 and nrow >= 1, got {padding} / {nrow}')
    T, H, W, dev = t0.T, t0.H, t0.W, t0.device
    CH, CW, xmaps, ymaps, pad = grid_shape(K, H, W, nrow, int(padding), border)
    out = torch.empty((T, CH, CW, 3) if layout == 'hwc' else (T, 3, CH, CW), dtype=dtype, device=dev)
    if T == 0:
        return out
    if dev.type == 'cuda':
        arr = (L.sf_egress_tile * len(tiles))()
        for i, t in enumerate(tiles):
            e = t.entry()
            e.history_len = t.border[1] if t.border is not None else 0
            arr[i] = e
        L.check(L.lib().sf_egress_grid(arr, len(tiles), out.data_ptr(), _GRID_MODE[(dtype, layout)], T, H, W, K if nrow is None else int(nrow),
                                       int(padding), float(pad_value), border, stream(out)))
        return out
    # the CPU home: the same float32 operations, tile by tile
    TH, TW = H + 2 * border, W + 2 * border
    canvas = torch.full((T, 3, CH, CW), float(pad_value), dtype=torch.float32)
    k = 0
    for t in tiles:
        rgb = t.rgb()                                        # [T, count, 3, H, W]
        for n in range(t.count):
            tile = rgb[:, n]
            if border:
                framed = torch.zeros(T, 3, TH, TW)
                hist = max(0, min(T, t.border[1]))
                framed[:hist, 1] = 0.7                       # green before history_len,
                framed[hist:, 0] = 0.7                       # red from it on
                framed[:, :, border:border + H, border:border + W] = tile
                tile = framed
            y0 = (k // xmaps) * (TH + pad) + pad
            x0 = (k % xmaps) * (TW + pad) + pad
            canvas[:, :, y0:y0 + TH, x0:x0 + TW] = tile
            k += 1
    if dtype == torch.float32:
        return canvas
    q = (canvas * 255.).clamp(0, 255).to(torch.uint8)
    out.copy_(q.permute(0, 2, 3, 1) if layout == 'hwc' else q)
    return out


# ---- (c) boxes -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def draw_boxes_(frames_u8, boxes, pres_mask=None, palette=None, width=2):
    """Rectangle outlines IN PLACE on uint8 CHW frames [F, 3, H, W]; returns frames_u8.  boxes [F, M, 4] float32 (x0, y0, x1, y1), pres_mask None
    or [F, M] (bool or uint8), palette [P, 3] uint8 (default: vp_utils.PALETTE_np).  Per frame the boxes that are present and have x0 >= 0 are kept
    and their coordinates truncated toward zero; the k-th KEPT box takes colour k (vp_vis.py:60-65 zips PALETTE[:N] with the surviving boxes: the
    rank after filtering, not the slot index; beyond the palette: its last colour).  A pixel belongs to an outline iff it lies inside the inclusive
    box and within `width` pixels of one of its four sides; outlines are clipped to the image and later boxes overwrite earlier ones.
    This is PIL's ImageDraw.rectangle(outline=, width=) -- what torchvision's draw_bounding_boxes calls -- for every box whose two sides are both
    >= 2 * width, boxes partly outside the image included.  The one difference: for thinner boxes PIL draws outside the box; this does not."""
    _check(frames_u8, 'frames to draw on', (torch.uint8, ), '[F, 3, H, W]', frames_u8.dim() == 4 and frames_u8.shape[1] == 3)
    F, _, H, W = frames_u8.shape
    _check(boxes, 'boxes', (torch.float32, ), f'[{F}, M, 4]', boxes.dim() == 3 and boxes.shape[0] == F and boxes.shape[2] == 4)
    M = boxes.shape[1]
    if M > MAX_BOXES or int(width) < 1:
        raise ValueError(f'slotformer_amd.egress: at most {MAX_BOXES} boxes per frame and width >= 1, got {M} / {width}')
    if boxes.device != frames_u8.device:
        raise ValueError(f'slotformer_amd.egress: frames and boxes live on {frames_u8.device} and {boxes.device}')
    if pres_mask is not None:
        _check(pres_mask, 'the presence mask', (torch.bool, torch.uint8), f'[{F}, {M}]', tuple(pres_mask.shape) == (F, M))
        pres_mask = pres_mask.to(device=frames_u8.device, dtype=torch.uint8)
    pal = _palette(palette, frames_u8.device)
    if F == 0 or M == 0 or H == 0 or W == 0:
        return frames_u8
    if frames_u8.is_cuda:
        L.check(L.lib().sf_egress_draw_boxes(frames_u8.data_ptr(), boxes.data_ptr(), ptr(pres_mask),
                                             pal.data_ptr(), pal.shape[0], F, M, H, W, int(width), stream(frames_u8)))
        return frames_u8
    ys = torch.arange(H).view(H, 1)
    xs = torch.arange(W).view(1, W)
    w = int(width)
    for f in range(F):
        keep = boxes[f, :, 0] >= 0.
        if pres_mask is not None:
            keep &= pres_mask[f] != 0
        for k, (x0, y0, x1, y1) in enumerate(boxes[f][keep].to(torch.int64).tolist()):   # (float -> int64 truncates toward zero)
            inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
            edge = (xs - x0 < w) | (x1 - xs < w) | (ys - y0 < w) | (y1 - ys < w)
            m = inside & edge
            colour = pal[min(k, pal.shape[0] - 1)]
            for c in range(3):
                frames_u8[f, c][m] = colour[c]
    return frames_u8
