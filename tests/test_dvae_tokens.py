"""CPU: what of the device tokeniser can be checked without a GPU -- the pack order of the head weight (the _host twin against the header's index
formula), the token files of slot_io, the argument errors of the new entry points, and the premise of the GPU tests: every case they use has at
most 2 % of its positions closer to a tie than the comparison rule resolves (tests/dvae_token_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dvae_token_cases as tc


def lib():
    from slotformer_amd import _lib
    return _lib.lib()


def err():
    return lib().sf_last_error_string().decode()


# ---- pack order ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [32, 64, 4096])
def test_pack_order_of_the_head_weight(V):
    w = torch.randn(V, 64, generator=tc.gen(V)) * 3
    w[0, 0], w[V - 1, 63] = 0., -1e-30   # a zero and a value whose remainder underflows
    nb = lib().sf_dvae_head_packed_bytes(V, 64)
    assert nb == V * 64 * 4
    buf = np.zeros(nb // 2, dtype=np.uint16)
    assert lib().sf_dvae_pack_head_weights_host(w.numpy().ctypes.data, buf.ctypes.data, V, 64) == 0, err()
    got = torch.from_numpy(buf.astype(np.int32)).view(2, V // 32, 4, 64, 8)
    assert torch.equal(got, tc.packed_expected(w))
    # hi + lo restores the weight to 2^-16 of its size (what split-bf16 carries)
    hi = (got[0] << 16).view(torch.float32)
    lo = (got[1] << 16).view(torch.float32)
    l = torch.arange(64)
    back = torch.empty(V, 64)
    for ks in range(4):
        for j in range(8):
            back[(32 * torch.arange(V // 32)[:, None] + (l & 31)[None]), (16 * ks + 8 * (l >> 5) + j)[None]] = (hi + lo)[:, ks, :, j]
    assert (back - w).abs().max() <= 2.**-16 * w.abs().max()


def test_shape_rule():
    ok = lib().sf_dvae_tokens_ok
    assert ok(4096, 64, 3, 128, 128) == 1 and ok(64, 64, 3, 64, 64) == 1 and ok(32, 64, 3, 4, 4) == 1 and ok(4096, 64, 3, 20, 36) == 1
    assert ok(100, 64, 3, 64, 64) == 0      # V no multiple of the MFMA block
    assert ok(0, 64, 3, 64, 64) == 0 and ok((1 << 20) + 32, 64, 3, 64, 64) == 0
    assert ok(4096, 128, 3, 64, 64) == 0    # K
    assert ok(4096, 64, 1, 64, 64) == 0     # C
    assert ok(4096, 64, 3, 66, 64) == 0 and ok(4096, 64, 3, 64, 30) == 0 and ok(4096, 64, 3, 0, 64) == 0
    assert lib().sf_dvae_head_packed_bytes(100, 64) == 0 and lib().sf_dvae_head_packed_bytes(64, 32) == 0


def test_argument_errors_without_gpu():
    """negative codes with a message, raised before any HIP call"""
    L = lib()
    one = C.c_void_p(16)    # a non-null, 16-byte aligned dummy pointer: every case below is rejected before it is dereferenced
    odd = C.c_void_p(20)
    assert L.sf_dvae_head_argmax_f32(None, 64, one, one, one, None, 8, 64, 64, None) < 0 and 'null pointer' in err()
    assert L.sf_dvae_head_argmax_f32(one, 64, one, one, None, None, 8, 64, 64, None) < 0 and 'null pointer' in err()
    assert L.sf_dvae_head_argmax_f32(one, 64, one, one, one, None, 8, 100, 64, None) < 0 and 'multiple of 32' in err()
    assert L.sf_dvae_head_argmax_f32(one, 64, one, one, one, None, 8, 64, 32, None) < 0 and 'K must be 64' in err()
    assert L.sf_dvae_head_argmax_f32(one, 64, one, one, one, one, 8, 32768 + 32, 64, None) < 0 and 'int16' in err()
    assert L.sf_dvae_head_argmax_f32(one, 63, one, one, one, None, 8, 64, 64, None) < 0 and 'row stride' in err()
    assert L.sf_dvae_head_argmax_f32(one, 66, one, one, one, None, 8, 64, 64, None) < 0 and 'row stride' in err()
    assert L.sf_dvae_head_argmax_f32(one, 64, one, one, one, None, -1, 64, 64, None) < 0 and 'row count' in err()
    assert L.sf_dvae_head_argmax_f32(odd, 64, one, one, one, None, 8, 64, 64, None) < 0 and 'aligned' in err()
    assert L.sf_dvae_patch_embed_f32(None, one, one, 1, 3, 8, 8, None) < 0 and 'null pointer' in err()
    assert L.sf_dvae_patch_embed_f32(one, one, one, 1, 1, 8, 8, None) < 0 and 'multiples of 4' in err()
    assert L.sf_dvae_patch_embed_f32(one, one, one, 1, 3, 10, 8, None) < 0 and 'multiples of 4' in err()
    assert L.sf_dvae_patch_embed_f32(one, one, one, -1, 3, 8, 8, None) < 0 and 'frame count' in err()
    assert L.sf_dvae_patch_embed_f32(odd, one, one, 1, 3, 8, 8, None) < 0 and 'aligned' in err()
    assert L.sf_dvae_pack_head_weights(None, one, 64, 64, None) < 0 and 'null pointer' in err()
    assert L.sf_dvae_pack_head_weights(one, one, 48, 64, None) < 0 and 'multiple of 32' in err()
    assert L.sf_dvae_pack_head_weights_host(one, None, 64, 64) < 0 and 'null pointer' in err()
    assert L.sf_dvae_pack_head_weights_host(one, one, 64, 48) < 0 and 'K must be 64' in err()


def test_no_cpu_fallback():
    from slotformer_amd import ops
    m = tc.seeded_dvae(64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.tokenize_ids(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.patch_embed(torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pack_head_weight(torch.zeros(64, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.linear_argmax(torch.zeros(4, 64), torch.zeros(64 * 64 * 4, dtype=torch.uint8), None, 64)
    assert ops.dvae_tokens_ok(4096, 64, 3, 128, 128) and not ops.dvae_tokens_ok(100, 64, 3, 128, 128)


# ---- token files ---------------------------------------------------------------------------------------------------------------------------------
def test_token_path():
    from slotformer_amd import slot_io
    assert (slot_io.token_path('/d/Physion/PhysionTrainMP4s/Collide/pilot_it2_0001_img.mp4', 'dvae_physion_params') ==
            '/d/Physion/PhysionTrainNpys-dvae_physion_params/Collide/pilot_it2_0001_img.npy')
    assert slot_io.token_path('/d/Physion/PhysionTestMP4s/x/7.mp4', 'dv') == '/d/Physion/PhysionTestNpys-dv/x/7.npy'
    # the dataset names a video by its frame folder: the same file
    assert slot_io.token_path('/d/Physion/PhysionTestMP4s/x/7', 'dv') == '/d/Physion/PhysionTestNpys-dv/x/7.npy'


def test_token_files_round_trip(tmp_path):
    from slotformer_amd import slot_io
    rs = np.random.RandomState(3)
    files = [str(tmp_path / 'PhysionTrainMP4s' / 'Drop' / f'{i}.mp4') for i in range(2)] + [str(tmp_path / 'PhysionTestMP4s' / 'Roll' / '0.mp4')]
    tokens = rs.randint(0, 4096, size=(3, 9, 16)).astype(np.int64)
    tokens[0, 0, 0], tokens[0, 0, 1] = 0, 32767
    written = slot_io.save_video_tokens(files, torch.from_numpy(tokens), 'dv')
    assert written == [slot_io.token_path(f, 'dv') for f in files] and all(os.path.exists(p) for p in written)
    assert written[2] == str(tmp_path / 'PhysionTestNpys-dv' / 'Roll' / '0.npy')
    on_disk = np.load(written[1])
    assert on_disk.dtype == np.int16 and on_disk.shape == (9, 16) and np.array_equal(on_disk, tokens[1])
    assert sorted(os.listdir(os.path.dirname(written[0]))) == ['0.npy', '1.npy']   # no temporary file left behind
    # the strided clip: frames 1, 4, 7
    clip = slot_io.read_token_clip(written[0], 1, 3, 3)
    assert clip.dtype == np.int32 and clip.shape == (3, 16) and np.array_equal(clip, tokens[0, [1, 4, 7]])
    assert int(clip.max()) <= 32767 and slot_io.read_token_clip(written[0], 0, 1, 1)[0, 1] == 32767
    # a missing file is no error: the dataset leaves `token_id` out
    assert slot_io.read_token_clip(str(tmp_path / 'PhysionTrainNpys-dv' / 'Drop' / '5.npy'), 0, 2, 1) is None
    # resume: an existing file is skipped (its content stays), a missing one is written
    os.remove(written[1])
    again = slot_io.save_video_tokens(files, tokens + 1, 'dv')
    assert again == [written[1]]
    assert np.array_equal(np.load(written[0]), tokens[0]) and np.array_equal(np.load(written[1]), tokens[1] + 1)
    assert len(slot_io.save_video_tokens(files, tokens, 'dv', overwrite=True)) == 3 and np.array_equal(np.load(written[1]), tokens[1])
    with pytest.raises(ValueError, match='int16'):
        slot_io.save_video_tokens([str(tmp_path / 'PhysionTrainMP4s' / 'Drop' / '9.mp4')], np.full((1, 2, 4), 40000), 'dv')
    with pytest.raises(ValueError, match=r'\[T, h\*w\]'):
        slot_io.save_video_tokens([str(tmp_path / 'PhysionTrainMP4s' / 'Drop' / '9.mp4')], np.zeros((1, 2, 2, 2), dtype=np.int16), 'dv')


# ---- the premise of the GPU tests ----------------------------------------------------------------------------------------------------------------
def unsafe_fraction(safe):
    return float((~safe).sum()) / safe.numel()


@pytest.mark.parametrize('V', tc.HEAD_VOCABS)
def test_premise_head_cases(V):
    for R in tc.HEAD_ROWS:
        c = tc.head_rows(V, R)
        n = int((~c['safe']).sum())
        print(f'head V {V} R {R}: {n} unsafe positions, {c["ids"].unique().numel()} distinct winners')
        assert n <= tc.MAX_UNSAFE * R, (V, R, n)
        assert c['x'].min() >= 0


def test_premise_planted_winner():
    c = tc.planted_case()
    assert torch.equal(c['ids'], c['c']) and bool(c['safe'].all())        # in float64 the planted column wins every row, away from a tie
    assert torch.equal(torch.sort(c['c']).values, torch.arange(4096))     # and every column is some row's winner


@pytest.mark.parametrize('V', [64, 4096])
def test_premise_ties(V):
    c = tc.tie_case(V)
    lg = c['logits']
    seen = set()
    for r, (what, idx) in enumerate(c['groups']):
        assert not seen & set(idx), what
        seen |= set(idx)
        assert all(0 <= i < V for i in idx) and list(idx) == sorted(idx)
        assert all(lg[r, i] == lg[r, idx[0]] for i in idx), what            # exact ties
        others = lg[r].clone()
        others[list(idx)] = -float('inf')
        assert lg[r, idx[0]] - others.max() > tc.SAFE_REL * lg.abs().max(), what   # and the maximum of the row, away from the rest


@pytest.mark.parametrize('V,F_,H,W', tc.MODEL_CASES)
def test_premise_model_cases(V, F_, H, W):
    c = tc.model_case(V, F_, H, W)
    n = int((~c['safe']).sum())
    print(f'encoder V {V}, {F_} frames {H} x {W}: {n} unsafe of {c["safe"].numel()}, {c["ids"].unique().numel()} distinct ids')
    assert n <= tc.MAX_UNSAFE * c['safe'].numel()
    # the load_state_dict test: the same frames under the weights of a second seed
    if (V, H) == (4096, 64):
        with torch.no_grad():
            ids1, safe1 = tc.judge(tc.encoder64(tc.model_case(V, F_, H, W, 1)['sd'], c['img']))
        assert unsafe_fraction(safe1) <= tc.MAX_UNSAFE and not torch.equal(ids1, c['ids'])


def test_premise_head_without_bias():
    c = tc.head_rows(512, 257)
    _, safe = tc.judge(c['x'][:256].double() @ c['w'].double().t())
    assert unsafe_fraction(safe) <= tc.MAX_UNSAFE


def test_premise_fixture():
    import golden_util as gu
    g = gu.load_golden('steve_tokens')
    safe = g['dvae_margin'] > tc.SAFE_REL * float(np.abs(g['dvae_logits']).max())
    assert (~safe).sum() <= tc.MAX_UNSAFE * safe.size


def test_patch_emulation_is_close_to_float64():
    for case in tc.PATCH_CASES:
        c = tc.patch_case(*case)
        assert 0 < tc.rel(c['emu'], c['ref']) < 1e-5 and tc.patch_bound(c) < tc.PARITY   # the bound comes from the arithmetic, not from the bar
