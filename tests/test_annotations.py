"""CPU: the run-length codec of slotformer_amd.annotations and the host path of `ground_truth` against the reference's computation written out
(tests/annotation_cases.py restate).  Everything is integer-exact: equality, no tolerance.

The cases run at a downscale (24 x 36 -> 8 x 8, a non-integer ratio) and at an upscale (5 x 7 -> 16 x 16).  Two properties hold at one size only
by construction: a 5 x 7 mask has 35 pixels, so its checkerboard has 35 runs (the one at 24 x 36 has more than 256), and nothing vanishes under
an upscale (the single pixel of 'vanish' is dropped at the downscale only)."""
import numpy as np
import pytest
import torch

import annotation_cases as AC


def A():
    from slotformer_amd import annotations
    return annotations


def ingest_for(kind):
    from slotformer_amd.ingest import FrameIngest
    return FrameIngest(AC.SIZES[kind][1])


LITERALS = [([0, 1, 4, 2, 2, 2, 2, 2, 5], '0141N0003'), ([20], 'd0'), ([0, 70000, 3, 5, 70000, 1], '0`[T23edkM][T2L')]


def test_literal_strings():
    a = A()
    m = np.zeros((4, 5), np.uint8)
    m[1:3, 1:4] = 1
    m[0, 0] = 1
    assert AC.encode(m)['counts'] == LITERALS[0][0]
    for runs, s in LITERALS:
        total = sum(runs)
        size = [1, total]
        for form in (s, s.encode()):
            got = a.rle_counts({'size': size, 'counts': form})
            assert got.dtype == np.uint32 and got.tolist() == runs, (s, got)
        assert a.rle_string(runs) == s
        assert a.rle_counts({'size': size, 'counts': runs}).tolist() == runs
    assert a.rle_of_mask(m) == {'size': [4, 5], 'counts': '0141N0003'}


def test_random_masks_round_trip():
    a = A()
    rs = np.random.RandomState(5)
    first_zero = 0
    for i in range(2000):
        h, w = rs.randint(1, 41, 2)
        kind = i % 10
        if kind == 0:
            m = np.zeros((h, w), np.uint8)
        elif kind == 1:
            m = np.ones((h, w), np.uint8)
        else:
            m = (rs.rand(h, w) < rs.choice([0.05, 0.5, 0.9])).astype(np.uint8)
            if kind == 2:
                m[0, 0] = 1   # the first run (of zeros) is empty
        obj = AC.encode(m)
        runs = obj['counts']
        first_zero += runs[0] == 0
        s = a.rle_string(runs)
        assert a.rle_counts({'size': obj['size'], 'counts': s}).tolist() == runs
        assert a.rle_string(a.rle_counts({'size': obj['size'], 'counts': s})) == s
        assert a.rle_of_mask(m) == {'size': obj['size'], 'counts': s}
        assert np.array_equal(AC.decode({'size': obj['size'], 'counts': a.rle_counts({'size': obj['size'], 'counts': s}).tolist()}), m)
    assert first_zero >= 200


def test_malformed_masks_raise():
    a = A()
    good = {'size': [4, 5], 'counts': '0141N0003'}
    assert a.rle_counts(good).sum() == 20
    for bad in ({'size': [4, 6], 'counts': '0141N0003'},            # the runs do not sum to h * w
                {'size': [4, 5], 'counts': [0, 1, 4, 2, 2, 2, 2, 2, 4]},
                {'size': [4, 5], 'counts': '0141N000' + chr(48 + 0x23)},   # the last group announces another one
                {'size': [4, 5], 'counts': [25, -5]},                 # a negative run
                {'size': [4, 5], 'counts': 'd0N'},                    # decodes to [20, 0, -2]
                {'size': [4, 5], 'counts': '01 41'},                  # outside the alphabet
                {'size': [4, 5], 'counts': None}, {'counts': [20]}, {'size': [0, 5], 'counts': []}):
        with pytest.raises(ValueError):
            a.rle_counts(bad)
    with pytest.raises(ValueError):
        a.pack_frames([[good, {'size': [5, 4], 'counts': [20]}]])    # two sizes in one call
    with pytest.raises(ValueError):
        a.pack_frames([[], []])                                       # no object and no size


def compare(kind, name, form=None):
    a = A()
    frames, max_n = AC.cases(kind)[name]
    (h, w), size = AC.SIZES[kind]
    given = frames
    if form == 'string':
        given = [[{'size': o['size'], 'counts': a.rle_string(o['counts'])} for o in f] for f in frames]
    packed = a.pack_frames(given, size=(h, w))
    got = a.ground_truth(packed, ingest_for(kind), max_n_objects=max_n, device='cpu')
    mask, pres, bbox = AC.restate(frames, size, max_n + 1)
    T = len(frames)
    assert got['mask'].dtype == torch.int64 and got['pres_mask'].dtype == torch.bool and got['bbox'].dtype == torch.float32
    assert tuple(got['mask'].shape) == (T, ) + size and tuple(got['pres_mask'].shape) == (T, max_n + 1) and tuple(got['bbox'].shape) == (T, max_n + 1, 4)
    assert np.array_equal(got['mask'].numpy(), mask), (kind, name)
    assert np.array_equal(got['pres_mask'].numpy(), pres), (kind, name)
    assert np.array_equal(got['bbox'].numpy(), bbox), (kind, name)
    return got, packed


@pytest.mark.parametrize('kind', list(AC.SIZES))
@pytest.mark.parametrize('name', ['overlap', 'inside', 'vanish', 'borders', 'one_pixel', 'checkerboard', 'no_objects', 'fifteen', 'clip'])
def test_ground_truth_cpu(kind, name):
    got, packed = compare(kind, name)
    mask, pres = got['mask'].numpy(), got['pres_mask'].numpy()
    if name == 'inside':        # object 2 lies inside object 1: a box, no label pixel
        assert pres[0, :3].all() and not (mask == 2).any() and (mask == 3).sum() >= 1
    if name == 'vanish':
        assert (mask == 3).any() and pres[0].sum() == (2 if kind == 'down' else 3) and ((mask == 2).any() == (kind == 'up'))
    if name == 'borders':
        b = got['bbox'].numpy()[0]
        H, W = AC.SIZES[kind][1]
        assert b[0].tolist() == [0, 0, W - 1, H - 1] and b[1].tolist() == [0, 0, W - 1, H - 1]
    if name == 'one_pixel':
        assert pres[0].sum() == 1 and (mask == 1).sum() >= 1
    if name == 'checkerboard':
        runs = packed.object_offsets[2] - packed.object_offsets[1]
        assert runs > 256 if kind == 'down' else runs == 35
    if name == 'no_objects':
        assert not mask[0].any() and not pres[0].any() and not got['bbox'].numpy()[0].any() and (mask[1] == 1).all()
    if name == 'fifteen':
        assert pres[0].all() and sorted(set(mask.reshape(-1).tolist())) == list(range(16))


@pytest.mark.parametrize('kind', list(AC.SIZES))
def test_input_forms(kind):
    """compressed strings, [B, T] nesting, uint8 labels, a nested list given directly, frame ranges of a record"""
    a = A()
    ref, packed = compare(kind, 'clip')
    got, _ = compare(kind, 'clip', 'string')
    assert all(torch.equal(got[k], ref[k]) for k in ref)
    frames = AC.cases(kind)['clip'][0]
    ing = ingest_for(kind)
    bt = a.ground_truth([frames[:2], frames[2:]], ing, mask_dtype=torch.uint8)
    assert bt['mask'].dtype == torch.uint8 and tuple(bt['mask'].shape[:2]) == (2, 2) and tuple(bt['bbox'].shape) == (2, 2, 7, 4)
    assert all(torch.equal(bt[k].flatten(0, 1).to(ref[k].dtype), ref[k]) for k in ref)
    sub = a.ground_truth(packed.frames(1, 4), ing)
    assert all(torch.equal(sub[k], ref[k][1:4]) for k in ref)


def test_c_entries_reject_bad_arguments():
    """before any device work, so without a GPU (as tests/test_abi.py does for the other entries)"""
    import ctypes as C
    from slotformer_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)
    assert lib.sf_rle_label_maps(one, one, None, one, one, None, one, 1, 1, 1, 4, 5, 8, 8, None) < 0 and b'null pointer' in lib.sf_last_error_string()
    assert lib.sf_rle_label_maps(one, one, one, one, one, None, one, 1, 1, 1, 4, 20000, 8, 8, None) < 0 and b'16384' in lib.sf_last_error_string()
    assert lib.sf_rle_boxes_pad(one, one, one, one, 1, 65, None) < 0 and b'num' in lib.sf_last_error_string()
    assert lib.sf_rle_boxes_pad(one, one, one, None, 1, 7, None) < 0
    assert lib.sf_rle_label_maps(one, one, one, one, one, None, one, 0, 0, 0, 4, 5, 8, 8, None) == 0   # no frames: nothing to do


@pytest.mark.parametrize('kind', list(AC.SIZES))
def test_too_many_objects_raise(kind):
    a = A()
    (h, w), size = AC.SIZES[kind]
    fifteen = AC.cases(kind)['fifteen'][0][0]
    with pytest.raises(ValueError, match='at most 15'):
        a.pack_frames([fifteen + [AC.encode(AC.rect(h, w, 0, h, 0, w))]])
    # fifteen objects survive the resize, seven rows: the reference's pad fails with a shape error, this raises
    with pytest.raises(ValueError):
        AC.restate([fifteen], size, 7)
    with pytest.raises(ValueError, match='non-empty objects'):
        a.ground_truth([fifteen], ingest_for(kind), max_n_objects=6)
    assert a.ground_truth([fifteen], ingest_for(kind), max_n_objects=14)['pres_mask'].all()
