"""The annotation cases tests/test_annotations.py and tests/test_annotations_gpu.py share: run-length masks built from small dense masks, and the
restatement of the reference's CLEVRER ground truth (anno2mask, process_mask, masks_to_boxes_pad, argmax) they are compared against."""
import functools

import numpy as np
import torch

SIZES = {'down': ((24, 36), (8, 8)), 'up': ((5, 7), (16, 16))}   # (h, w) -> (H, W): a non-integer ratio down, an upscale


def encode(mask):
    """dense [h, w] -> the annotation dict, encoded HERE (column-major runs, uncompressed) so the cases do not lean on the package's encoder"""
    m = np.asarray(mask) != 0
    flat = m.T.reshape(-1)
    runs, cur, n = [], False, 0
    for v in flat:
        if bool(v) != cur:
            runs.append(n)
            cur, n = bool(v), 0
        n += 1
    runs.append(n)
    return {'size': [int(m.shape[0]), int(m.shape[1])], 'counts': runs}


def decode(obj):
    h, w = obj['size']
    flat = np.zeros(h * w, np.uint8)
    at, val = 0, 0
    for r in obj['counts']:   # (the cases hold the uncompressed form)
        flat[at:at + int(r)] = val
        at, val = at + int(r), 1 - val
    return flat.reshape(w, h).T


def nearest_index(n_in, n_out):
    """the source index F.interpolate(mode='nearest') reads for every output index of one axis"""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return torch.nn.functional.interpolate(src, size=(n_out, 1), mode='nearest').view(-1).long().numpy()


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def pixel(h, w, y, x):
    return rect(h, w, y, y + 1, x, x + 1)


@functools.lru_cache(maxsize=None)
def cases(kind):
    """name -> (frames [T] of per-frame mask-dict lists, max_n_objects)"""
    (h, w), (H, W) = SIZES[kind]
    ry, cx = nearest_index(h, H), nearest_index(w, W)
    seen = np.zeros((h, w), bool)
    seen[np.ix_(ry, cx)] = True
    sy, sx = int(ry[len(ry) // 2]), int(cx[len(cx) // 2])   # a source pixel the resize reads
    enc = lambda *ms: [encode(m) for m in ms]   # noqa: E731
    out = {}
    out['overlap'] = ([enc(rect(h, w, 0, h // 2 + 1, 0, w // 2 + 1), rect(h, w, h // 3, h, w // 3, w))], 6)
    out['inside'] = ([enc(rect(h, w, 0, h, 0, w // 2), rect(h, w, 1, h // 2, 1, w // 2 - 1), rect(h, w, 0, h, w // 2, w))], 6)
    # object 1 is a single pixel: under the downscale the resize does not read it (boxes shift up, label 3 stays 3)
    lone = (1, 1)
    assert kind == 'up' or not seen[lone]
    out['vanish'] = ([enc(rect(h, w, 0, h // 3, 0, w), pixel(h, w, *lone), rect(h, w, h // 2, h, w // 2, w))], 6)
    ring_a, ring_b = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    ring_a[0, :], ring_a[:, 0] = 1, 1
    ring_b[h - h // 3:, :], ring_b[:, w - w // 3:] = 1, 1   # (thick enough for the downscale to read it)
    out['borders'] = ([enc(ring_a, ring_b)], 6)
    out['one_pixel'] = ([enc(pixel(h, w, sy, sx))], 6)
    board = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(np.uint8)
    out['checkerboard'] = ([enc(rect(h, w, 0, 2, 0, 2), board, rect(h, w, h - 2, h, w - 2, w))], 6)
    out['no_objects'] = ([[], enc(rect(h, w, 0, h, 0, w)), []], 6)
    cells = [(y, x) for y in ry[::2] for x in cx[::2]][:15] if kind == 'down' else [(y, x) for y in range(h) for x in range(w)][::2][:15]
    cells = list(dict.fromkeys((int(y), int(x)) for y, x in cells))
    assert len(cells) == 15
    out['fifteen'] = ([enc(*[pixel(h, w, y, x) for y, x in cells])], 14)
    # three frames that differ, one record
    out['clip'] = ([out['overlap'][0][0], [], out['vanish'][0][0], out['checkerboard'][0][0]], 6)
    return out


def restate(frames, size, num):
    """The reference's computation, written out: dense column-major decode, background = not any, F.interpolate(mode='nearest') per channel,
    boxes as min / max of nonzero, the filter, compact and pad, argmax(0).  A frame without objects (which the reference cannot stack) gives
    zeros.  More than `num` surviving objects: ValueError (the reference's shape error)."""
    H, W = size
    masks, press, boxes = [], [], []
    for f in frames:
        bbox, pres = np.zeros((num, 4), np.float32), np.zeros(num, bool)
        if not f:
            masks.append(np.zeros((H, W), np.int64))
            press.append(pres)
            boxes.append(bbox)
            continue
        m = np.stack([decode(o) for o in f], 0).astype(np.int32)
        m = np.concatenate([np.logical_not(np.any(m, axis=0))[None], m], 0)
        t = torch.from_numpy(m).float()
        t = torch.stack([torch.nn.functional.interpolate(c[None, None], size=(H, W), mode='nearest')[0, 0] for c in t], 0).long()
        obj = t[1:]
        obj = obj[obj.sum([-1, -2]) > 0]
        if obj.shape[0] > num:
            raise ValueError('more surviving objects than num')
        for k, o in enumerate(obj):
            ys, xs = torch.nonzero(o, as_tuple=True)
            bbox[k] = (xs.min().item(), ys.min().item(), xs.max().item(), ys.max().item())
            pres[k] = True
        masks.append(t.argmax(0).numpy())
        press.append(pres)
        boxes.append(bbox)
    return np.stack(masks), np.stack(press), np.stack(boxes)
