"""The device side of the data hand-over: raw uint8 frames as a decoder produced them -> the normalised, resized float32 frames the first
convolution reads (the reference's `BaseTransforms`, base_slots/datasets/utils.py:15-43: ToTensor, Normalize, Resize), its nearest-neighbour mask
resizing (`process_mask`) and PHYRE's class-index-to-colour lookup (datasets/phyre.py:50) -- csrc/ingest.hip.

Same functions, both homes (the vp_utils.py pattern): device tensors go to the kernels on the current stream, CPU tensors take a plain-torch path
that applies the SAME host-built float64 tables, so the two agree to float32 rounding.  File I/O and decoding stay with the caller.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._call import stream

BILINEAR, ANTIALIAS, NEAREST = 0, 1, 2


def resolve_size(resolution, H0, W0):
    """(H, W) for a source of H0 x W0: a pair is taken as it is; an int is torchvision's rule 'smaller edge to this size', the other edge
    int(size * long / short)."""
    if isinstance(resolution, (tuple, list)):
        if len(resolution) == 2:
            return int(resolution[0]), int(resolution[1])
        if len(resolution) != 1:
            raise ValueError(f'resolution must be an int or (H, W), got {resolution!r}')
        resolution = resolution[0]
    size = int(resolution)
    short, long = (W0, H0) if W0 <= H0 else (H0, W0)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if W0 <= H0 else (new_short, new_long)


def host_tables(H0, W0, H, W, mode):
    """The table of (H0, W0) -> (H, W) in `mode` as the library builds it on the host (float64 coordinates, float32 weights): a dict of numpy
    arrays, rows 'ry_first' [H], 'ry_count' [H], 'ry_w' [H, tapsY] and columns 'cx_first' [W], 'cx_count' [W], 'cx_w' [W, tapsX], plus 'blob',
    the int32 words the kernels read."""
    lib = L.lib()
    nbytes = lib.sf_ingest_tables_bytes(H0, W0, H, W, mode)
    if nbytes == 0:
        raise ValueError(f'slotformer_amd.ingest: no table for {H0} x {W0} -> {H} x {W}, mode {mode}')
    blob = np.zeros(nbytes // 4, dtype=np.int32)
    L.check(lib.sf_ingest_tables_host(blob.ctypes.data_as(C.c_void_p), nbytes, H0, W0, H, W, mode))
    ty, tx = int(blob[6]), int(blob[7])
    o = 8
    t = {'blob': blob, 'tapsY': ty, 'tapsX': tx}
    for name, n, taps in (('ry', H, ty), ('cx', W, tx)):
        t[name + '_first'] = blob[o:o + n]
        t[name + '_count'] = blob[o + n:o + 2 * n]
        t[name + '_w'] = blob[o + 2 * n:o + 2 * n + n * taps].view(np.float32).reshape(n, taps)
        o += 2 * n + n * taps
    return t


def _dense(first, count, w, n_in):
    """the taps of one axis as a dense [out, in] float32 matrix (the CPU path)"""
    m = np.zeros((len(first), n_in), dtype=np.float32)
    for i, (f, c) in enumerate(zip(first, count)):
        m[i, f:f + c] = w[i, :c]
    return torch.from_numpy(m)


class FrameIngest:
    """FrameIngest(resolution, mean=(0.5,), std=(0.5,), antialias=False, palette=None)

    resolution: (H, W), or an int = 'smaller edge to this size' (torchvision's rule, resolved on the host per source size).  mean / std: one value or
    one per channel.  antialias=False is the reference's resize (bilinear, align_corners=False); True is F.interpolate(..., antialias=True), what newer
    torchvision applies to tensors by default.  palette: a [K, 3] uint8 colour table -- the sources are then [..., H0, W0] uint8 colour INDICES
    (PHYRE's observations; an index >= K takes colour K - 1).  No colour table is built in.  Tables are cached per source size on the object."""

    def __init__(self, resolution, mean=(0.5, ), std=(0.5, ), antialias=False, palette=None):
        self.resolution = resolution
        mean = [float(m) for m in (mean if isinstance(mean, (tuple, list)) else (mean, ))]
        std = [float(s) for s in (std if isinstance(std, (tuple, list)) else (std, ))]
        if len(mean) not in (1, 3) or len(std) not in (1, 3) or any(s == 0 for s in std):
            raise ValueError(f'slotformer_amd.ingest: mean / std take one value or three, std non-zero; got {mean} / {std}')
        self.mean = tuple(mean * (3 if len(mean) == 1 else 1))
        self.std = tuple(std * (3 if len(std) == 1 else 1))
        self.antialias = bool(antialias)
        self.palette = None
        if palette is not None:
            pal = torch.as_tensor(palette)
            if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
                raise ValueError(f'slotformer_amd.ingest: the palette is a [K, 3] uint8 table with 1 <= K <= 256, got {tuple(pal.shape)} {pal.dtype}')
            self.palette = pal.cpu().contiguous()
        self.max_blocks = 0       # > 0 caps the grid of the frame kernel (its workgroups then loop)
        self._tables = {}         # (H0, W0, H, W, mode) -> {'host': dict, device: tensor}
        self._consts = {}         # device -> palette copy
        self._mean3 = (C.c_float * 3)(*self.mean)
        self._std3 = (C.c_float * 3)(*self.std)

    # ---- shapes -----------------------------------------------------------------------------------------------------------------------
    def output_size(self, H0, W0):
        return resolve_size(self.resolution, H0, W0)

    def _tab(self, H0, W0, mode, device=None):
        H, W = self.output_size(H0, W0)
        key = (H0, W0, H, W, mode)
        ent = self._tables.get(key)
        if ent is None:
            ent = self._tables[key] = {'host': host_tables(H0, W0, H, W, mode)}
        if device is None:
            return ent['host'], H, W
        dkey = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if dkey not in ent:
            ent[dkey] = torch.from_numpy(ent['host']['blob']).to(device)   # uploaded once per (sizes, mode, device)
        return ent[dkey], H, W

    def _check_frames(self, frames):
        if not torch.is_tensor(frames):
            raise ValueError(f'slotformer_amd.ingest: frames must be a torch tensor, got {type(frames).__name__}')
        shape = tuple(frames.shape)
        if frames.dtype != torch.uint8:
            raise ValueError(f'slotformer_amd.ingest: frames must be uint8 as decoded, got {frames.dtype} {shape}')
        if self.palette is not None:
            if frames.dim() >= 3 and shape[-1] == 3:   # (an index image three pixels wide is read as RGB: not supported)
                raise ValueError(f'slotformer_amd.ingest: a palette takes colour indices [..., H0, W0], not a 3-channel source {shape}')
            if frames.dim() < 2:
                raise ValueError(f'slotformer_amd.ingest: colour indices are [..., H0, W0], got {shape}')
            lead, (H0, W0) = shape[:-2], shape[-2:]
        else:
            if frames.dim() < 3 or shape[-1] != 3:
                raise ValueError(f'slotformer_amd.ingest: frames are [..., H0, W0, 3] (HWC), got {shape}')
            lead, (H0, W0) = shape[:-3], shape[-3:-1]
        if H0 < 1 or W0 < 1:
            raise ValueError(f'slotformer_amd.ingest: empty frames {shape}')
        if not frames.is_contiguous():
            raise ValueError(f'slotformer_amd.ingest: frames must be contiguous, got shape {shape} with strides {tuple(frames.stride())}')
        return lead, H0, W0

    def output_shape(self, frames):
        """shape of ingest(frames)"""
        lead, H0, W0 = self._check_frames(frames)
        return tuple(lead) + (3, ) + self.output_size(H0, W0)

    # ---- frames -----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def ingest(self, frames, out=None):
        """uint8 [..., H0, W0, 3] (or [..., H0, W0] colour indices with a palette) -> float32 [..., 3, H, W] = resize((x / 255 - mean) / std).
        Device tensors: one kernel launch on the current stream.  CPU tensors: torch ops on the same tables.  out=: written and returned."""
        lead, H0, W0 = self._check_frames(frames)
        H, W = self.output_size(H0, W0)
        oshape = tuple(lead) + (3, H, W)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=frames.device)
        elif tuple(out.shape) != oshape or out.dtype != torch.float32 or out.device != frames.device or not out.is_contiguous():
            raise ValueError(f'slotformer_amd.ingest: out must be a contiguous float32 tensor {oshape} on {frames.device}, got '
                             f'{tuple(out.shape)} {out.dtype} on {out.device}')
        F = int(np.prod(lead)) if len(lead) else 1
        if F == 0:
            return out
        mode = ANTIALIAS if self.antialias else BILINEAR
        if frames.is_cuda:
            tab, _, _ = self._tab(H0, W0, mode, frames.device)
            pal, K = None, 0
            if self.palette is not None:
                dkey = (frames.device.type, frames.device.index)
                if dkey not in self._consts:
                    self._consts[dkey] = self.palette.to(frames.device)
                pal, K = self._consts[dkey].data_ptr(), self.palette.shape[0]
            L.check(L.lib().sf_ingest_frames_u8(frames.data_ptr(), pal, K, tab.data_ptr(), self._mean3, self._std3, out.data_ptr(), F, H0, W0, H, W,
                                                mode, int(self.max_blocks), stream(frames)))
            return out
        t, _, _ = self._tab(H0, W0, mode)
        if 'wy' not in t:
            t['wy'] = _dense(t['ry_first'], t['ry_count'], t['ry_w'], H0)
            t['wx'] = _dense(t['cx_first'], t['cx_count'], t['cx_w'], W0)
        if self.palette is not None:
            x = self.palette[frames.reshape(F, H0, W0).long().clamp_(max=self.palette.shape[0] - 1)]   # [F, H0, W0, 3]
        else:
            x = frames.reshape(F, H0, W0, 3)
        x = x.float()
        rows = torch.matmul(t['wy'], x.reshape(F, H0, W0 * 3)).reshape(F, H, W0, 3).permute(0, 3, 1, 2)   # [F, 3, H, W0]
        res = torch.matmul(rows, t['wx'].t())                                                               # [F, 3, H, W]
        a = torch.tensor([1.0 / (255.0 * s) for s in self.std], dtype=torch.float32).view(1, 3, 1, 1)
        b = torch.tensor([-m / s for m, s in zip(self.mean, self.std)], dtype=torch.float32).view(1, 3, 1, 1)
        out.view(F, 3, H, W).copy_(res * a + b)
        return out

    __call__ = ingest

    # ---- masks ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def process_mask(self, mask, dtype=None):
        """BaseTransforms.process_mask: [H0, W0] or [N, H0, W0] ids, int64 or uint8 (a numpy array becomes int64, as in the reference) -> the same
        leading shape at the ingest resolution, nearest neighbour as F.interpolate(mode='nearest') picks it.  dtype: torch.int64 / torch.uint8 of
        the result (default: the source's)."""
        if isinstance(mask, np.ndarray):
            mask = torch.from_numpy(mask).long()
        if not torch.is_tensor(mask) or mask.dtype not in (torch.int64, torch.uint8) or mask.dim() not in (2, 3):
            raise ValueError(f'slotformer_amd.ingest: a mask is [H0, W0] or [N, H0, W0], int64 or uint8, got '
                             f'{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__} {getattr(mask, "dtype", "")}')
        dtype = mask.dtype if dtype is None else dtype
        if dtype not in (torch.int64, torch.uint8):
            raise ValueError(f'slotformer_amd.ingest: masks come out as int64 or uint8, not {dtype}')
        if not mask.is_contiguous():
            raise ValueError(f'slotformer_amd.ingest: masks must be contiguous, got shape {tuple(mask.shape)} with strides {tuple(mask.stride())}')
        H0, W0 = mask.shape[-2:]
        F = mask.shape[0] if mask.dim() == 3 else 1
        if mask.is_cuda:
            tab, H, W = self._tab(H0, W0, NEAREST, mask.device)
            out = torch.empty(tuple(mask.shape[:-2]) + (H, W), dtype=dtype, device=mask.device)
            if F:
                L.check(L.lib().sf_resize_masks_nearest(mask.data_ptr(), int(mask.dtype == torch.uint8), tab.data_ptr(),
                                                        out.data_ptr() if dtype == torch.int64 else None, out.data_ptr() if dtype == torch.uint8 else None,
                                                        F, H0, W0, H, W, stream(mask)))
            return out
        t, H, W = self._tab(H0, W0, NEAREST)
        ry = torch.from_numpy(t['ry_first'].astype(np.int64))
        cx = torch.from_numpy(t['cx_first'].astype(np.int64))
        return mask.index_select(-2, ry).index_select(-1, cx).to(dtype).contiguous()
