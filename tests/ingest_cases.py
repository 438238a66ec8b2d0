"""Shared by tests/test_ingest.py and tests/test_ingest_gpu.py: the shape list and the float64 yardstick of the ingest path."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# (H0, W0) -> (H, W): the smallest shapes where the resampling can go wrong
SHAPES = [
    ((29, 37), (16, 24)),      # odd row length; a frame is 3219 bytes, so every later frame starts misaligned; non-representable ratio
    ((29, 37), (29, 37)),      # identity: weights are 0 / 1
    ((50, 70), (64, 64)),      # upsampling: negative source coordinates clamp
    ((320, 480), (128, 128)),  # CLEVRER
    ((320, 480), (64, 64)),    # the widest antialias footprint
    ((5, 7), (40, 56)),        # source smaller than one band; non-square output
]
PALETTE_SHAPE = ((256, 256), (128, 128))   # PHYRE: colour indices
NFRAMES = 5
BOUND = 4e-6        # |kernel - float64| on outputs in [-1, 1]: a few dozen roundings of 2^-24 on values <= 1
TABLE_BOUND = 2e-7  # float32 rounding of the weights alone


def yardstick(u8, size, antialias, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """torch on the CPU in float64: u8 [F, H0, W0, 3] -> [F, 3, H, W]"""
    m = torch.tensor(mean, dtype=torch.float64)
    s = torch.tensor(std, dtype=torch.float64)
    x = ((u8.double() / 255 - m) / s).permute(0, 3, 1, 2)
    return F.interpolate(x, size, mode='bilinear', align_corners=False, antialias=bool(antialias))


@functools.lru_cache(maxsize=None)
def frames_of(H0, W0, seed=0):
    """NFRAMES random frames [F, H0, W0, 3] uint8 (computed once; do not write to them)"""
    rs = np.random.RandomState(1000 * H0 + W0 + seed)
    return torch.from_numpy(rs.randint(0, 256, size=(NFRAMES, H0, W0, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def reference_of(H0, W0, H, W, antialias):
    """the yardstick of frames_of(H0, W0) (computed once, shared between the tests; do not write to it)"""
    return yardstick(frames_of(H0, W0), (H, W), antialias)


@functools.lru_cache(maxsize=None)
def palette_case():
    """(indices [F, 256, 256] uint8 with some ids >= K, palette [7, 3] uint8, the RGB frames the lookup gives)"""
    rs = np.random.RandomState(77)
    (H0, W0), _ = PALETTE_SHAPE
    pal = torch.from_numpy(rs.randint(0, 256, size=(7, 3), dtype=np.uint8))
    idx = torch.from_numpy(rs.randint(0, 9, size=(NFRAMES, H0, W0), dtype=np.uint8))   # 7 and 8 are past the table: colour 6
    rgb = pal[idx.long().clamp(max=6)]
    return idx, pal, rgb
