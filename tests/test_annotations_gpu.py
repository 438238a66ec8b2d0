"""GPU: the run-length kernels (csrc/rle_masks.hip) through annotations.ground_truth against its host path, which tests/test_annotations.py holds
to the reference's computation.  Integer results: exact equality.  Every input is validated on the host: no malformed array reaches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

import annotation_cases as AC

pytestmark = pytest.mark.gpu

NAMES = ['overlap', 'inside', 'vanish', 'borders', 'one_pixel', 'checkerboard', 'no_objects', 'fifteen', 'clip']


def ingest_for(kind):
    from slotformer_amd.ingest import FrameIngest
    return FrameIngest(AC.SIZES[kind][1])


def same(dev_out, cpu_out):
    for k in ('mask', 'pres_mask', 'bbox'):
        assert dev_out[k].is_cuda and dev_out[k].dtype == cpu_out[k].dtype and dev_out[k].shape == cpu_out[k].shape, k
        assert torch.equal(dev_out[k].cpu(), cpu_out[k]), k


@pytest.mark.parametrize('mask_dtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('kind', list(AC.SIZES))
def test_device_equals_host(dev, kind, mask_dtype):
    from slotformer_amd import annotations as a
    ing = ingest_for(kind)
    (h, w), _ = AC.SIZES[kind]
    for name in NAMES:
        frames, max_n = AC.cases(kind)[name]
        packed = a.pack_frames(frames, size=(h, w))
        same(a.ground_truth(packed, ing, max_n_objects=max_n, device=dev, mask_dtype=mask_dtype),
             a.ground_truth(packed, ing, max_n_objects=max_n, device='cpu', mask_dtype=mask_dtype))


@pytest.mark.parametrize('kind', list(AC.SIZES))
def test_batched_input_frame_ranges_and_a_side_stream(dev, kind):
    from slotformer_amd import annotations as a
    ing = ingest_for(kind)
    frames = AC.cases(kind)['clip'][0]
    nested = [frames[:2], frames[2:], frames[1:3]]   # [B = 3][T = 2]
    want = a.ground_truth(nested, ing)
    assert tuple(want['mask'].shape[:2]) == (3, 2)
    same(a.ground_truth(nested, ing, device=dev), want)
    packed = a.pack_frames(nested)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = a.ground_truth(packed, ing, device=dev, check=False)           # (no synchronisation inside)
        part = a.ground_truth(packed.frames(2, 5), ing, device=dev, check=False)
    side.synchronize()
    same(got, want)
    same(part, {k: v.flatten(0, 1)[2:5] for k, v in want.items()})


def test_more_survivors_than_boxes_raise(dev):
    from slotformer_amd import annotations as a
    for kind in AC.SIZES:
        fifteen = AC.cases(kind)['fifteen'][0]
        with pytest.raises(ValueError, match='non-empty objects'):
            a.ground_truth(fifteen, ingest_for(kind), max_n_objects=6, device=dev)
        # unchecked: the first seven boxes, every label
        got = a.ground_truth(fifteen, ingest_for(kind), max_n_objects=6, device=dev, check=False)
        full = a.ground_truth(fifteen, ingest_for(kind), max_n_objects=14)
        assert torch.equal(got['mask'].cpu(), full['mask']) and torch.equal(got['bbox'].cpu(), full['bbox'][:, :7]) and got['pres_mask'].all()


def test_runs_beyond_the_lds_window(dev):
    """An object with more run ends than the kernel stages in LDS is searched in global memory, and so is every object behind it; the object in
    front of it is searched in LDS.  The window's size is read from the kernel's source."""
    from slotformer_amd import annotations as a
    from slotformer_amd.ingest import FrameIngest
    src = open(os.path.join(os.path.dirname(a.__file__), 'csrc', 'rle_masks.hip')).read()
    window = int(re.search(r'constexpr int kLdsRuns = (\d+);', src).group(1))
    h = w = int(np.ceil(np.sqrt(window + 64)))
    board = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(np.uint8)
    front, behind = AC.rect(h, w, 0, h // 4, 0, w // 4), AC.rect(h, w, h // 2, h, w // 2, w)
    frames = [[AC.encode(front), AC.encode(board), AC.encode(behind)], [AC.encode(behind), AC.encode(front)], [AC.encode(board)]]
    packed = a.pack_frames(frames)
    assert packed.object_offsets[2] - packed.object_offsets[1] > window
    for size in ((32, 32), (h + 3, w + 5)):
        ing = FrameIngest(size)
        for dtype in (torch.int64, torch.uint8):
            same(a.ground_truth(packed, ing, device=dev, mask_dtype=dtype), a.ground_truth(packed, ing, mask_dtype=dtype))
    want = AC.restate(frames, (32, 32), 7)
    got = a.ground_truth(packed, FrameIngest((32, 32)), device=dev)
    assert np.array_equal(got['mask'].cpu().numpy(), want[0]) and np.array_equal(got['pres_mask'].cpu().numpy(), want[1])
    assert np.array_equal(got['bbox'].cpu().numpy(), want[2])
