"""CPU: the ingest path (slotformer_amd/ingest.py, csrc/ingest.hip) without a GPU -- the host-built float64 tables, the plain-torch path of
FrameIngest, mask resizing, the palette lookup, the argument errors and the smaller-edge rule -- against torch on the CPU in float64:
F.interpolate(((u8.double() / 255 - mean) / std).permute(...), size, mode='bilinear', align_corners=False, antialias=a)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ingest_cases as ic

ALL_SHAPES = ic.SHAPES + [ic.PALETTE_SHAPE]


def _apply_tables_f64(t, x):
    """x [F, H0, W0, 3] float64 -> [F, 3, H, W] float64 with the table's taps, in float64 NumPy"""
    H, W = len(t['ry_first']), len(t['cx_first'])
    rows = np.zeros((x.shape[0], H, x.shape[2], 3))
    for y in range(H):
        f, c = int(t['ry_first'][y]), int(t['ry_count'][y])
        rows[:, y] = np.tensordot(t['ry_w'][y, :c].astype(np.float64), x[:, f:f + c], axes=([0], [1]))
    out = np.zeros((x.shape[0], H, W, 3))
    for xo in range(W):
        f, c = int(t['cx_first'][xo]), int(t['cx_count'][xo])
        out[:, :, xo] = np.tensordot(rows[:, :, f:f + c], t['cx_w'][xo, :c].astype(np.float64), axes=([2], [0]))
    return out.transpose(0, 3, 1, 2)


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('src,dst', ALL_SHAPES)
def test_host_tables(src, dst, antialias):
    """The exported host table function through ctypes: indices inside the source, taps summing to 1, and the tables applied in float64
    reproducing the yardstick to the float32 rounding of the weights."""
    from slotformer_amd import ingest
    (H0, W0), (H, W) = src, dst
    t = ingest.host_tables(H0, W0, H, W, antialias)
    for ax, n_in in (('ry', H0), ('cx', W0)):
        first, count, w = t[ax + '_first'], t[ax + '_count'], t[ax + '_w']
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all(), ax
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), ax   # (bands rely on monotone tables)
        assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= ic.TABLE_BOUND, ax
        assert all((w[i, count[i]:] == 0).all() for i in range(len(first))), ax
    u8 = ic.frames_of(H0, W0)[:2]
    got = _apply_tables_f64(t, ((u8.double() / 255 - 0.5) / 0.5).numpy())
    ref = ic.reference_of(H0, W0, H, W, antialias)[:2].numpy()
    err = np.abs(got - ref).max()
    print(f'tables {src}->{dst} aa={antialias}: taps {t["tapsY"]} x {t["tapsX"]}, max err {err:.2e}')
    assert err <= ic.TABLE_BOUND


def test_identity_tables_are_zero_one():
    from slotformer_amd import ingest
    t = ingest.host_tables(29, 37, 29, 37, 0)
    assert (t['ry_first'] == np.arange(29)).all() and (t['ry_w'][:, 0] == 1).all() and (t['ry_w'][:, 1:] == 0).all()
    assert (t['cx_first'] == np.arange(37)).all() and (t['cx_w'][:, 0] == 1).all()


def test_table_arguments():
    import ctypes as C
    from slotformer_amd import _lib
    lib = _lib.lib()
    assert lib.sf_ingest_tables_bytes(0, 4, 4, 4, 0) == 0 and lib.sf_ingest_tables_bytes(4, 4, 4, 4, 3) == 0
    n = lib.sf_ingest_tables_bytes(5, 7, 40, 56, 1)
    buf = (C.c_int * (n // 4))()
    assert lib.sf_ingest_tables_host(buf, n - 4, 5, 7, 40, 56, 1) < 0 and b'smaller' in lib.sf_last_error_string()
    assert lib.sf_ingest_tables_host(None, n, 5, 7, 40, 56, 1) < 0 and b'null pointer' in lib.sf_last_error_string()
    assert lib.sf_ingest_tables_host(buf, n, 5, 7, 40, 56, 1) == 0 and list(buf[1:6]) == [5, 7, 40, 56, 1]
    assert n == 4 * (8 + (2 + buf[6]) * 40 + (2 + buf[7]) * 56)
    # the kernels' argument checks come before any device work
    one = C.c_void_p(16)
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (C.c_float * 3)(0.5, 0.0, 0.5)
    assert lib.sf_ingest_frames_u8(one, None, 0, None, m3, m3, one, 1, 5, 7, 40, 56, 0, 0, None) < 0 and b'null pointer' in lib.sf_last_error_string()
    assert lib.sf_ingest_frames_u8(one, None, 0, one, m3, z3, one, 1, 5, 7, 40, 56, 0, 0, None) < 0 and b'std' in lib.sf_last_error_string()
    assert lib.sf_ingest_frames_u8(one, one, 300, one, m3, m3, one, 1, 5, 7, 40, 56, 0, 0, None) < 0 and b'palette' in lib.sf_last_error_string()
    assert lib.sf_ingest_frames_u8(one, None, 0, one, m3, m3, one, 1, 5, 7, 40, 56, 2, 0, None) < 0
    assert lib.sf_ingest_frames_u8(one, None, 0, one, m3, m3, one, 1, 64, 16384, 1, 1, 1, 0, None) < 0 and b'LDS' in lib.sf_last_error_string()
    assert lib.sf_resize_masks_nearest(one, 0, one, None, None, 1, 5, 7, 40, 56, None) < 0
    assert lib.sf_resize_masks_nearest(one, 0, one, one, None, 1, 5, 0, 40, 56, None) < 0


@pytest.mark.parametrize('antialias', [False, True])
@pytest.mark.parametrize('src,dst', ic.SHAPES)
def test_torch_path_matches_float64(src, dst, antialias):
    from slotformer_amd.ingest import FrameIngest
    u8 = ic.frames_of(*src)
    ing = FrameIngest(dst, antialias=antialias)
    got = ing.ingest(u8)
    ref = ic.reference_of(*src, *dst, int(antialias))
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = (got.double() - ref).abs().max().item()
    print(f'torch path {src}->{dst} aa={antialias}: max err {err:.2e}')
    assert err <= ic.BOUND
    # leading dimensions, out=, per-channel statistics
    mean, std = (0.4, 0.5, 0.6), (0.6, 0.5, 0.7)
    ing2 = FrameIngest(dst, mean=mean, std=std, antialias=antialias)
    clip = u8[:4].reshape(2, 2, *u8.shape[1:])
    out = torch.full((2, 2, 3) + tuple(dst), 9.)
    assert ing2(clip, out=out) is out
    ref2 = ic.yardstick(u8[:4], dst, antialias, mean, std).reshape(2, 2, 3, *dst)
    assert (out.double() - ref2).abs().max().item() <= ic.BOUND


@pytest.mark.parametrize('antialias', [False, True])
def test_palette_lookup(antialias):
    from slotformer_amd.ingest import FrameIngest
    idx, pal, rgb = ic.palette_case()
    (H0, W0), dst = ic.PALETTE_SHAPE
    assert (idx >= 7).any()    # indices past the table take its last colour
    ing = FrameIngest(dst, antialias=antialias, palette=pal)
    got = ing.ingest(idx)
    ref = ic.yardstick(rgb, dst, antialias)
    assert got.shape == (ic.NFRAMES, 3) + dst and (got.double() - ref).abs().max().item() <= ic.BOUND
    # a palette given as a numpy array or a list is the same table
    assert torch.equal(FrameIngest(dst, antialias=antialias, palette=pal.numpy()).ingest(idx[:1]), got[:1])


@pytest.mark.parametrize('src,dst', [((320, 480), (128, 128)), ((5, 7), (64, 64)), ((29, 37), (29, 37)), ((29, 37), (16, 24))])
def test_process_mask_is_interpolate_nearest(src, dst):
    from slotformer_amd.ingest import FrameIngest
    rs = np.random.RandomState(5)
    ing = FrameIngest(dst)
    m3 = torch.from_numpy(rs.randint(0, 256, size=(3, ) + src)).long()
    ref = F.interpolate(m3[None].double(), dst, mode='nearest')[0].long()
    got = ing.process_mask(m3)
    assert got.dtype == torch.int64 and torch.equal(got, ref)
    assert torch.equal(ing.process_mask(m3[0]), ref[0])                       # [H0, W0] -> [H, W]
    assert torch.equal(ing.process_mask(m3.numpy().astype(np.int32)), ref)    # a numpy array becomes int64, as in the reference
    u8 = ing.process_mask(m3.to(torch.uint8))
    assert u8.dtype == torch.uint8 and torch.equal(u8.long(), ref)
    assert torch.equal(ing.process_mask(m3, dtype=torch.uint8), u8) and torch.equal(ing.process_mask(m3.to(torch.uint8), dtype=torch.int64), ref)


def test_value_errors():
    from slotformer_amd.ingest import FrameIngest
    ing = FrameIngest((16, 24))
    u8 = ic.frames_of(29, 37)
    with pytest.raises(ValueError, match=r'uint8.*\(5, 29, 37, 3\)'):
        ing.ingest(u8.float())
    with pytest.raises(ValueError, match=r'\(5, 29, 37, 4\)'):
        ing.ingest(torch.zeros(5, 29, 37, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'\(29, 37\)'):
        ing.ingest(torch.zeros(29, 37, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'contiguous.*\(5, 29, 19, 3\)'):
        ing.ingest(u8[:, :, ::2])
    with pytest.raises(ValueError, match=r'contiguous'):
        ing.ingest(u8.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match=r'out must be.*\(5, 3, 16, 24\)'):
        ing.ingest(u8, out=torch.empty(5, 3, 16, 25))
    pal = torch.zeros(7, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r'palette.*\(5, 29, 37, 3\)'):
        FrameIngest((16, 24), palette=pal).ingest(u8)
    with pytest.raises(ValueError, match=r'palette'):
        FrameIngest((16, 24), palette=torch.zeros(7, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'palette'):
        FrameIngest((16, 24), palette=torch.zeros(7, 3))
    with pytest.raises(ValueError):
        FrameIngest((16, 24), std=(0.5, 0., 0.5))
    with pytest.raises(ValueError, match=r'mask'):
        ing.process_mask(torch.zeros(2, 3, 29, 37, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'mask'):
        ing.process_mask(torch.zeros(29, 37))
    with pytest.raises(ValueError, match=r'contiguous'):
        ing.process_mask(torch.zeros(3, 29, 37, dtype=torch.int64)[:, :, ::2])


def test_int_resolution_is_the_smaller_edge():
    from slotformer_amd.ingest import FrameIngest, resolve_size
    assert resolve_size(128, 320, 480) == (128, 192)     # landscape: the height is the smaller edge
    assert resolve_size(128, 480, 320) == (192, 128)     # portrait
    assert resolve_size(64, 50, 70) == (64, 89)          # int(64 * 70 / 50) = 89 (truncated, torchvision's rule)
    assert resolve_size(64, 64, 64) == (64, 64)
    assert resolve_size((16, 24), 29, 37) == (16, 24)
    u8 = ic.frames_of(50, 70)
    got = FrameIngest(64).ingest(u8)
    assert got.shape == (ic.NFRAMES, 3, 64, 89)
    assert (got.double() - ic.yardstick(u8, (64, 89), False)).abs().max().item() <= ic.BOUND
    assert FrameIngest(64).process_mask(torch.zeros(50, 70, dtype=torch.uint8)).shape == (64, 89)
