"""Annotation masks -> the ground truth of the video-prediction evaluation, on the device.

The reference's CLEVRER dataset builds `mask`, `pres_mask` and `bbox` per frame on the CPU when `load_mask` is set (base_slots/datasets/clevrer.py:
101-125, datasets/utils.py:46-77): it decodes the COCO run-length masks of `derender_proposals` with pycocotools, resizes them with nearest
neighbour, takes boxes with torchvision.ops.masks_to_boxes, compacts and pads them, and takes the argmax over [background, objects...].  Here the
run lengths are parsed on the host (pure Python / NumPy), packed, and expanded by two kernels (csrc/rle_masks.hip) straight at the ingest
resolution: no dense mask at source size exists anywhere.  `ground_truth(..., device='cpu')` is the same computation in NumPy.

Two departures from the reference, both documented where they happen: a frame without objects is allowed (labels all 0, no present box; the
reference's np.stack of an empty list raises), and more surviving objects than `max_n_objects + 1` raise ValueError (the reference fails with a
shape error in masks_to_boxes_pad).
"""
import numpy as np
import torch

from . import _lib as L
from . import ingest as _ingest

MAX_OBJECTS = 15   # per frame: the metric kernels take ground-truth ids in [0, 16)
MAX_BOXES = 64     # sf_rle_boxes_pad, sf_vp_bbox_pr_f32


# ---- the codec -------------------------------------------------------------------------------------------------------------------------

def _size_of(obj):
    try:
        h, w = (int(v) for v in obj['size'])
    except (KeyError, TypeError, ValueError):
        raise ValueError(f'slotformer_amd.annotations: a mask is {{"size": [h, w], "counts": ...}}, got {obj!r}') from None
    if h < 1 or w < 1 or h * w >= 2**32:
        raise ValueError(f'slotformer_amd.annotations: a mask has at least one pixel and fewer than 2^32, got {h} x {w}')
    return h, w


def rle_counts(obj):
    """The run lengths of one annotation mask {'size': [h, w], 'counts': ...} as uint32.  Runs alternate 0, 1, 0, ... starting with a run of
    ZEROS (possibly empty), over the mask in column-major order (pixel (y, x) at index x * h + y).  `counts` is a list of ints (the uncompressed
    form) or COCO's compressed string (str or bytes): one value per run in 5-bit groups, least significant group first, each character
    48 + (group | 0x20 if more groups follow); bit 0x10 of the last group is the sign and is extended; from the fourth run on the stored value
    is counts[i] - counts[i - 2].  Raises ValueError for a truncated string, a character outside the alphabet, a negative run, or runs that do
    not sum to h * w: nothing malformed reaches a kernel.

    pycocotools is not a dependency and was not available to compare against: fidelity to its `mask.decode` rests on the format description
    above (its rleFrString / rleToString), not on a run of that package."""
    h, w = _size_of(obj)
    counts = obj.get('counts')
    if isinstance(counts, str):
        counts = counts.encode('ascii', errors='replace')
    if isinstance(counts, (bytes, bytearray)):
        # every character at once: value index, place inside the value, the groups shifted and summed per value
        c = np.frombuffer(bytes(counts), dtype=np.uint8).astype(np.int64) - 48
        if c.size and (c.min() < 0 or c.max() > 63):
            raise ValueError('slotformer_amd.annotations: a character outside the run-length alphabet')
        more = (c & 0x20) != 0
        if c.size and more[-1]:
            raise ValueError('slotformer_amd.annotations: truncated run-length string (a group announces another one at the end)')
        last = np.flatnonzero(~more)
        first = np.concatenate([[0], last[:-1] + 1]) if last.size else last
        place = np.arange(c.size) - np.repeat(first, last - first + 1)
        if c.size and place.max() > 7:
            raise ValueError('slotformer_amd.annotations: a run of more than 40 bits')
        x = np.add.reduceat((c & 0x1f) << (5 * place), first) if last.size else np.zeros(0, np.int64)
        x = x - (((c[last] & 0x10) != 0) * (np.int64(1) << (5 * (last - first + 1))))
        # from the fourth run on the string holds counts[i] - counts[i - 2]: sums along the odd and along the even runs
        x[1::2] = np.cumsum(x[1::2])
        x[2::2] = np.cumsum(x[2::2])
        runs = x
    elif isinstance(counts, (list, tuple, np.ndarray)):
        try:
            given = np.asarray(counts)
            runs = given.astype(np.int64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError('slotformer_amd.annotations: run lengths are integers') from None
        if runs.ndim != 1 or (runs.size and not np.array_equal(runs, given)):
            raise ValueError('slotformer_amd.annotations: run lengths are a flat list of integers')
    else:
        raise ValueError(f'slotformer_amd.annotations: counts are a list of ints, a str or bytes, got {type(counts).__name__}')
    if runs.size and runs.min() < 0:
        raise ValueError('slotformer_amd.annotations: negative run length')
    if runs.size and runs.max() > h * w or int(runs.sum()) != h * w:
        raise ValueError(f'slotformer_amd.annotations: the runs cover {int(runs.sum())} pixels, the mask has {h} x {w} = {h * w}')
    return runs.astype(np.uint32)


def rle_string(counts):
    """The inverse of `rle_counts` for the compressed form: run lengths -> COCO's string (str)."""
    runs = [int(v) for v in counts]
    if any(r < 0 for r in runs):
        raise ValueError('slotformer_amd.annotations: negative run length')
    out = bytearray()
    for i, x in enumerate(runs):
        if i > 2:
            x -= runs[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append(48 + (c | 0x20 if more else c))
    return out.decode('ascii')


def rle_of_mask(mask):
    """A dense [h, w] mask (nonzero = covered) -> {'size': [h, w], 'counts': <compressed string>}: for fixtures and tests."""
    m = np.asarray(mask) != 0
    if m.ndim != 2:
        raise ValueError(f'slotformer_amd.annotations: a mask is [h, w], got {m.shape}')
    flat = m.T.reshape(-1)   # column-major
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    runs = np.diff(edges).tolist()
    if flat.size and flat[0]:
        runs = [0] + runs
    return {'size': [int(m.shape[0]), int(m.shape[1])], 'counts': rle_string(runs)}


# ---- packing ---------------------------------------------------------------------------------------------------------------------------

class PackedFrames:
    """The run lengths of F frames as three flat arrays: `run_ends` uint32 [R], the CUMULATIVE run ends of every object one after the other (run
    j of an object covers the column-major indices [end[j - 1], end[j]); odd j = covered); `object_offsets` int32 [O + 1], the first run of every
    object; `frame_offsets` int32 [F + 1], the first object of every frame; `h`, `w`, the source size; `lead`, the leading shape ((B, T) or
    (T, )) of the nested list they came from."""

    def __init__(self, run_ends, object_offsets, frame_offsets, h, w, lead):
        self.run_ends, self.object_offsets, self.frame_offsets = run_ends, object_offsets, frame_offsets
        self.h, self.w, self.lead = int(h), int(w), tuple(int(v) for v in lead)
        self._dev = {}

    @property
    def num_frames(self):
        return len(self.frame_offsets) - 1

    def frames(self, start, stop, lead=None):
        """Frames [start, stop) as a record of their own that SHARES the run and object arrays (offsets stay absolute)."""
        if not 0 <= start <= stop <= self.num_frames:
            raise ValueError(f'slotformer_amd.annotations: frames [{start}, {stop}) of {self.num_frames}')
        sub = PackedFrames(self.run_ends, self.object_offsets, self.frame_offsets[start:stop + 1], self.h, self.w,
                           (stop - start, ) if lead is None else lead)
        sub._dev = {k: (e, o, f[start:stop + 1]) for k, (e, o, f) in self._dev.items()}
        return sub

    def on(self, device):
        """(run_ends, object_offsets, frame_offsets) on `device`, uploaded once."""
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            # (an empty array still gets an address the kernels may be handed)
            ends = self.run_ends if len(self.run_ends) else np.zeros(1, np.uint32)
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(device, non_blocking=True)
                                   for a in (ends, self.object_offsets, self.frame_offsets))
        return self._dev[key]


def _nest(frames):
    """nested list -> (flat list of frames, lead)"""
    if not isinstance(frames, (list, tuple)):
        raise ValueError(f'slotformer_amd.annotations: frames are a nested list [B][T] or [T] of per-frame object lists, got {type(frames).__name__}')
    is_frame = lambda f: isinstance(f, (list, tuple)) and all(isinstance(o, dict) for o in f)   # noqa: E731
    if all(is_frame(f) for f in frames):   # [T] (a list of empty lists is T frames without objects)
        return list(frames), (len(frames), )
    if all(isinstance(v, (list, tuple)) and all(is_frame(f) for f in v) for v in frames):
        T = len(frames[0])
        if any(len(v) != T for v in frames):
            raise ValueError('slotformer_amd.annotations: every video of a call has the same number of frames')
        return [f for v in frames for f in v], (len(frames), T)
    raise ValueError('slotformer_amd.annotations: frames are a nested list [B][T] or [T] of per-frame lists of mask dicts')


def pack_frames(frames, size=None):
    """frames: a nested list [B][T] or [T] of per-frame object lists -- the anno['frames'][i]['objects'][k]['mask'] dicts of a CLEVRER
    `derender_proposals` file, in annotation order -> PackedFrames.  All frames of a call share
    one size; `size` = (h, w) names it when no frame of the call has an object.  At most 15 objects per frame (the metric kernels take
    ground-truth ids in [0, 16)): more raises ValueError.  A frame WITHOUT objects is allowed -- labels all 0, no present box -- where the
    reference's np.stack of an empty list raises (datasets/utils.py:52)."""
    flat, lead = _nest(frames)
    hw = None if size is None else (int(size[0]), int(size[1]))
    ends, obj_off, frame_off = [], [0], [0]
    total = 0
    for f in flat:
        if len(f) > MAX_OBJECTS:
            raise ValueError(f'slotformer_amd.annotations: {len(f)} objects in a frame; the evaluation takes at most {MAX_OBJECTS} (ground-truth ids in [0, 16))')
        for o in f:
            runs = rle_counts(o)
            if hw is None:
                hw = _size_of(o)
            elif _size_of(o) != hw:
                raise ValueError(f'slotformer_amd.annotations: all frames of a call share one size; got {_size_of(o)} after {hw}')
            ends.append(np.cumsum(runs, dtype=np.uint64).astype(np.uint32))
            total += len(runs)
            obj_off.append(total)
        frame_off.append(len(obj_off) - 1)
    if hw is None:
        raise ValueError('slotformer_amd.annotations: no object in any frame: pass size=(h, w)')
    if not (1 <= hw[0] <= 16384 and 1 <= hw[1] <= 16384):
        raise ValueError(f'slotformer_amd.annotations: frame sizes lie in [1, 16384] (the resize tables), got {hw[0]} x {hw[1]}')
    if total >= 2**31:
        raise ValueError('slotformer_amd.annotations: too many runs for one record')
    return PackedFrames(np.concatenate(ends) if ends else np.zeros(0, np.uint32), np.asarray(obj_off, np.int32), np.asarray(frame_off, np.int32),
                        hw[0], hw[1], lead)


# ---- ground truth ----------------------------------------------------------------------------------------------------------------------

def _host_ground_truth(p, ry, cx, num, mask_dtype):
    F, H, W = p.num_frames, len(ry), len(cx)
    labels = np.zeros((F, H, W), np.int64)
    bbox = np.zeros((F, num, 4), np.float32)
    pres = np.zeros((F, num), bool)
    src = (cx.astype(np.int64)[None, :] * p.h + ry.astype(np.int64)[:, None]).reshape(-1)   # column-major source index of every output pixel
    for f in range(F):
        k = 0
        for n, o in enumerate(range(p.frame_offsets[f], p.frame_offsets[f + 1])):
            e = p.run_ends[p.object_offsets[o]:p.object_offsets[o + 1]]
            on = ((np.searchsorted(e, src, side='right') & 1) == 1).reshape(H, W)   # (the runs sum to h * w: the index stays below len(e))
            labels[f][on & (labels[f] == 0)] = n + 1
            if not on.any():
                continue   # empty AFTER the resize: dropped from the boxes; the label ids are not compacted (masks_to_boxes_pad vs argmax)
            if k >= num:
                raise ValueError(f'slotformer_amd.annotations: a frame has more than {num} non-empty objects (max_n_objects + 1)')
            ys, xs = np.nonzero(on)
            bbox[f, k] = (xs.min(), ys.min(), xs.max(), ys.max())
            pres[f, k] = True
            k += 1
    return torch.from_numpy(labels).to(mask_dtype), torch.from_numpy(pres), torch.from_numpy(bbox)


def ground_truth(frames_or_packed, ingest, max_n_objects=6, device=None, mask_dtype=torch.int64, check=True):
    """What the reference's CLEVRER dataset returns with load_mask (clevrer.py:101-125), at the resolution of `ingest` (a `FrameIngest`: its
    `output_size` and its nearest table -- F.interpolate(mode='nearest') as `process_mask` applies it -- fix (H, W)):

        'mask'      [..., H, W] mask_dtype (int64 or uint8): 1 + the first object of the frame, in annotation order, that covers the pixel's
                    source pixel, 0 where none does = argmax(0) over [not any(objects), objects...]
        'pres_mask' [..., max_n_objects + 1] bool, 'bbox' [..., max_n_objects + 1, 4] float32 [min x, min y, max x, max y]: the boxes of every
                    object's OWN resized mask (an object hidden behind an earlier one still has its box), objects that are empty after the
                    resize dropped, the rest compacted in order and padded with zeros.  The label ids are not compacted: the asymmetry is the
                    reference's.

    frames_or_packed: the nested list of `pack_frames`, or its PackedFrames; the leading shape [B, T] or [T] is the input's.  On a CUDA device:
    two launches on the current stream and no synchronisation, unless check=True (the default), which reads one flag word -- one
    synchronisation -- and raises ValueError when a frame has more non-empty objects than max_n_objects + 1 (with check=False such a frame keeps
    the first max_n_objects + 1 boxes).  device=None / 'cpu': the same computation in NumPy, with the same results."""
    p = frames_or_packed if isinstance(frames_or_packed, PackedFrames) else pack_frames(frames_or_packed)
    num = int(max_n_objects) + 1
    if not 1 <= num <= MAX_BOXES:
        raise ValueError(f'slotformer_amd.annotations: max_n_objects + 1 in [1, {MAX_BOXES}], got {num}')
    if mask_dtype not in (torch.int64, torch.uint8):
        raise ValueError(f'slotformer_amd.annotations: masks come out as int64 or uint8, not {mask_dtype}')
    device = torch.device('cpu' if device is None else device)
    if device.type == 'cuda':
        out, flag = device_ground_truth(p, ingest, max_n_objects, device, mask_dtype)
        if check and int(flag.item()):
            raise ValueError(f'slotformer_amd.annotations: a frame has more than {num} non-empty objects (max_n_objects + 1)')
        return out
    t, H, W = ingest._tab(p.h, p.w, _ingest.NEAREST)
    mask, pres, bbox = _host_ground_truth(p, t['ry_first'], t['cx_first'], num, mask_dtype)
    return {'mask': mask.view(p.lead + (H, W)), 'pres_mask': pres.view(p.lead + (num, )), 'bbox': bbox.view(p.lead + (num, 4))}


def device_ground_truth(p, ingest, max_n_objects, device, mask_dtype=torch.int64):
    """The device half of `ground_truth` for a PackedFrames: (its dict, the flag word [1] int32 on the device -- nonzero when a frame has more
    non-empty objects than max_n_objects + 1).  Two launches on the current stream, no synchronisation: a caller that chains calls ORs the flag
    words and reads them once."""
    num, F = int(max_n_objects) + 1, p.num_frames
    tab, H, W = ingest._tab(p.h, p.w, _ingest.NEAREST, device)
    mask = torch.empty(F, H, W, dtype=mask_dtype, device=device)
    bbox = torch.empty(F, num, 4, dtype=torch.float32, device=device)
    pres = torch.empty(F, num, dtype=torch.bool, device=device)
    flag = (torch.empty if F else torch.zeros)(1, dtype=torch.int32, device=device)   # (zeroed by sf_rle_boxes_pad)
    if F:
        ends, obj_off, frame_off = p.on(device)
        extents = torch.empty(F, MAX_OBJECTS, 5, dtype=torch.int32, device=device)
        st = torch.cuda.current_stream(device).cuda_stream
        lib = L.lib()
        L.check(lib.sf_rle_label_maps(ends.data_ptr(), obj_off.data_ptr(), frame_off.data_ptr(), tab.data_ptr(),
                                      mask.data_ptr() if mask_dtype == torch.int64 else None, mask.data_ptr() if mask_dtype == torch.uint8 else None,
                                      extents.data_ptr(), F, len(p.object_offsets) - 1, len(p.run_ends), p.h, p.w, H, W, st))
        L.check(lib.sf_rle_boxes_pad(extents.data_ptr(), bbox.data_ptr(), pres.data_ptr(), flag.data_ptr(), F, num, st))
    return {'mask': mask.view(p.lead + (H, W)), 'pres_mask': pres.view(p.lead + (num, )), 'bbox': bbox.view(p.lead + (num, 4))}, flag
