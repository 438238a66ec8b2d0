"""GPU: the device tokeniser (csrc/dvae_tokens.hip, dVAE.tokenize_ids, harness.extract_video_tokens) against the float64 restatements of
tests/dvae_token_cases.py.

Ids are compared by the project's safe rule (dvae_token_cases.check_ids): equal to float64 wherever the two best float64 logits are further apart
than 1e-4 x max|logit|, and overall no more differing positions than unsafe ones; tests/test_dvae_tokens.py asserts on the CPU that every case
used here has at most 2 % unsafe positions.  The patch embedding is held to four times the distance of a float32 emulation of split-bf16 from
float64, never above 1e-3.  Measured on an MI355X: profiles/tokenize.md."""
import numpy as np
import pytest
import torch

import dvae_token_cases as tc
import golden_util as gu

pytestmark = pytest.mark.gpu


def head_ids(dev, x, w, b, both=True):
    """(int64 ids, int16 ids) of the head kernel on device copies"""
    from slotformer_amd import ops
    V = w.shape[0]
    packed = ops.pack_head_weight(w.to(dev))
    R = x.shape[0]
    i64 = torch.full((R, ), -1, device=dev, dtype=torch.int64)
    i16 = torch.full((R, ), -1, device=dev, dtype=torch.int16)
    ops.linear_argmax(x, packed, None if b is None else b.to(dev), V, out=i64, out_i16=i16 if both else None)
    return i64, i16


def model_on(dev, c, V):
    m = tc.seeded_dvae(V)
    m.load_state_dict(c['sd'])
    return m.to(dev)


# ---- the head kernel -----------------------------------------------------------------------------------------------------------------------------
def test_pack_on_the_device_equals_the_host_twin(dev):
    from slotformer_amd import ops
    w = tc.head_case(512)['w']
    got = ops.pack_head_weight(w.to(dev)).cpu().view(torch.int16).to(torch.int32) & 0xffff
    assert torch.equal(got.view(2, 16, 4, 64, 8), tc.packed_expected(w))


@pytest.mark.parametrize('V', tc.HEAD_VOCABS)
@pytest.mark.parametrize('R', tc.HEAD_ROWS)
def test_head_matches_float64(dev, R, V):
    c = tc.head_rows(V, R)
    i64, i16 = head_ids(dev, c['x'].to(dev), c['w'], c['b'])
    diff, unsafe = tc.check_ids(i64, c['ids'], c['safe'])
    print(f'\nhead R {R} V {V}: {diff} positions differ from float64, {unsafe} unsafe')
    assert torch.equal(i16.long(), i64)
    # either output alone gives the same ids
    from slotformer_amd import ops
    packed = ops.pack_head_weight(c['w'].to(dev))
    only64 = ops.linear_argmax(c['x'].to(dev), packed, c['b'].to(dev), V)
    only16 = ops.linear_argmax(c['x'].to(dev), packed, c['b'].to(dev), V, out_i16=torch.empty(R, device=dev, dtype=torch.int16))
    assert only64.dtype == torch.int64 and torch.equal(only64, i64) and only16.dtype == torch.int16 and torch.equal(only16, i16)


@pytest.mark.parametrize('R', [65, 1000])
def test_head_takes_a_row_stride(dev, R):
    c = tc.head_rows(4096, R)
    buf = torch.full((R, tc.HEAD_LD), float('nan'), device=dev)   # what lies between the rows must never be read
    buf[:, :64] = c['x'].to(dev)
    i64, i16 = head_ids(dev, buf[:, :64], c['w'], c['b'])
    tc.check_ids(i64, c['ids'], c['safe'])
    dense, _ = head_ids(dev, c['x'].to(dev), c['w'], c['b'])
    assert torch.equal(i64, dense) and torch.equal(i16.long(), i64)


def test_head_without_bias_and_leading_dims(dev):
    from slotformer_amd import ops
    c = tc.head_rows(512, 257)
    x = c['x'][:256].reshape(4, 8, 8, 64).to(dev)
    ids = ops.linear_argmax(x, ops.pack_head_weight(c['w'].to(dev)), None, 512)
    want, safe = tc.judge(c['x'][:256].double() @ c['w'].double().t())
    assert ids.shape == (4, 8, 8)
    tc.check_ids(ids, want.view(4, 8, 8), safe.view(4, 8, 8))


def test_every_column_can_win(dev):
    c = tc.planted_case()
    i64, i16 = head_ids(dev, c['x'].to(dev), c['w'], None)
    assert torch.equal(i64.cpu(), c['c'])
    assert torch.equal(i16.long(), i64)


@pytest.mark.parametrize('V', [64, 4096])
def test_first_index_wins_a_tie(dev, V):
    c = tc.tie_case(V)
    i64, i16 = head_ids(dev, c['x'].to(dev), c['w'], c['b'])
    for r, (what, idx) in enumerate(c['groups']):
        assert int(i64[r]) == idx[0], f'{what}: indices {idx} tie, got {int(i64[r])}'
    assert torch.equal(i16.long(), i64)


def test_int16_refused_for_a_large_vocabulary(dev):
    from slotformer_amd import ops
    V = 32768 + 32
    w = torch.zeros(V, 64, device=dev)
    packed = ops.pack_head_weight(w)
    with pytest.raises(RuntimeError, match='int16'):
        ops.linear_argmax(torch.zeros(4, 64, device=dev), packed, None, V, out_i16=torch.empty(4, device=dev, dtype=torch.int16))
    ids = ops.linear_argmax(torch.zeros(4, 64, device=dev), packed, None, V)   # int64 is fine; all logits tie at 0: the first index
    assert torch.equal(ids.cpu(), torch.zeros(4, dtype=torch.int64))


# ---- patch embedding -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F_,H,W', tc.PATCH_CASES, ids=[f'{f}x{h}x{w}' for f, h, w in tc.PATCH_CASES])
def test_patch_embed_matches_float64(dev, F_, H, W):
    from slotformer_amd import ops
    c = tc.patch_case(F_, H, W)
    got = ops.patch_embed(c['img'].to(dev), c['w'].to(dev))
    d, bound = tc.rel(got, c['ref']), tc.patch_bound(c)
    print(f'\npatch embed {F_}x{H}x{W}: |device - float64| {d:.3e}  bound {bound:.3e}  (emulation {tc.rel(c["emu"], c["ref"]):.3e}, '
          f'device vs emulation {tc.rel(got, c["emu"]):.3e})')
    assert got.shape == (F_, H // 4, W // 4, 64) and got.dtype == torch.float32
    assert d <= bound


def test_patch_embed_ignores_the_precision_mode(dev, precision):
    from slotformer_amd import ops
    c = tc.patch_case(3, 20, 36)
    got = ops.patch_embed(c['img'].to(dev), c['w'].to(dev))
    from slotformer_amd import _lib
    old = _lib.lib().sf_get_precision()
    _lib.lib().sf_set_precision(1)
    try:
        assert torch.equal(got, ops.patch_embed(c['img'].to(dev), c['w'].to(dev)))
    finally:
        _lib.lib().sf_set_precision(old)


# ---- tokenize_ids --------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_tokenize_ids_on_the_reference_fixture(dev):
    """the reference's own dVAE ids (tests/golden/steve_tokens.npz), built as test_steve_image_side_golden builds the model"""
    from test_engine_gpu import build
    g = gu.load_golden('steve_tokens')
    m, _ = build(gu.steve_tokens_cfg(), g, 601, dev)
    img = gu.seeded_img(1, 2, 64, seed=602).to(dev)
    ids = m.dvae.tokenize_ids(img)
    assert ids.shape == (1, 2, 16, 16) and ids.dtype == torch.int64
    safe = torch.from_numpy(g['dvae_margin']) > tc.SAFE_REL * float(np.abs(g['dvae_logits']).max())
    diff, unsafe = tc.check_ids(ids[0], torch.from_numpy(g['dvae_ids']), safe)
    print(f'\nfixture: {diff} positions differ from the reference, {unsafe} unsafe')


@torch.no_grad()
@pytest.mark.parametrize('V,F_,H,W', tc.MODEL_CASES, ids=[f'V{v}-{f}x{h}x{w}' for v, f, h, w in tc.MODEL_CASES])
def test_tokenize_ids_matches_float64_and_tokenize(dev, V, F_, H, W):
    c = tc.model_case(V, F_, H, W)
    m = model_on(dev, c, V)
    img = c['img'].to(dev)
    ids = m.tokenize_ids(img)
    assert ids.shape == (F_, H // 4, W // 4) and ids.dtype == torch.int64
    diff, unsafe = tc.check_ids(ids, c['ids'], c['safe'])
    old = m.tokenize(img, one_hot=False)
    d_old, _ = tc.check_ids(old, c['ids'], c['safe'])                       # the unchanged path obeys the same rule ...
    d_both = int((ids != old).sum())
    assert torch.equal(ids.cpu()[c['safe']], old.cpu()[c['safe']]) and d_both <= unsafe   # ... so the two agree wherever float64 is decided
    print(f'\ntokenize_ids V {V} {F_}x{H}x{W}: {diff} differ from float64, tokenize {d_old}, from each other {d_both}; {unsafe} unsafe')
    # int16, and into a buffer of the caller's
    i16 = m.tokenize_ids(img, dtype=torch.int16)
    assert i16.dtype == torch.int16 and torch.equal(i16.long(), ids)
    buf = torch.full((F_ * (H // 4) * (W // 4), ), -1, device=dev, dtype=torch.int16)
    ret = m.tokenize_ids(img, out=buf, dtype=torch.int16)
    assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf.view_as(ids).long(), ids)


@torch.no_grad()
def test_tokenize_ids_5d_and_bitwise_independence(dev):
    c = tc.model_case(4096, 3, 64, 64)
    m = model_on(dev, c, 4096)
    img = c['img'].to(dev)
    ids = m.tokenize_ids(img).clone()
    assert torch.equal(ids, m.tokenize_ids(img))                                        # a second run
    for f in range(3):
        assert torch.equal(ids[f:f + 1], m.tokenize_ids(img[f:f + 1])), f               # a frame alone
    assert torch.equal(ids[[2, 0]], m.tokenize_ids(img[[2, 0]].contiguous()))           # other neighbours
    five = m.tokenize_ids(torch.stack([img, img.flip(0)], 0))                           # [B, T, ...]
    assert five.shape == (2, 3, 16, 16) and torch.equal(five[0], ids) and torch.equal(five[1], ids.flip(0))
    assert m.tokenize_ids(img[:, None]).shape == (3, 1, 16, 16)
    with pytest.raises(TypeError, match='dtype'):
        m.tokenize_ids(img, dtype=torch.int32)
    with pytest.raises(TypeError, match='out must be'):
        m.tokenize_ids(img, out=torch.empty(5, device=dev, dtype=torch.int64))


@torch.no_grad()
def test_refused_shape_returns_what_tokenize_returns(dev):
    from slotformer_amd import ops
    assert not ops.dvae_tokens_ok(100, 64, 3, 64, 64)
    m = tc.seeded_dvae(100).to(dev)
    img = tc.model_case(64, 2, 64, 64)['img'].to(dev)
    want = m.tokenize(img, one_hot=False)
    assert torch.equal(m.tokenize_ids(img), want)
    assert torch.equal(m.tokenize_ids(img[None]), want[None])
    i16 = m.tokenize_ids(img, dtype=torch.int16)
    assert i16.dtype == torch.int16 and torch.equal(i16.long(), want)
    buf = torch.empty(2, 16, 16, device=dev, dtype=torch.int64)
    assert m.tokenize_ids(img, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, want)


@torch.no_grad()
def test_packed_head_is_rebuilt_after_load_state_dict(dev):
    c0, c1 = tc.model_case(4096, 3, 64, 64), tc.model_case(4096, 3, 64, 64, 1)
    m = model_on(dev, c0, 4096)
    img = c0['img'].to(dev)
    a = m.tokenize_ids(img).clone()
    packed = m._head_packed()
    assert m._head_packed() is packed                      # kept while nothing changes
    m.load_state_dict(c1['sd'])
    assert m._head_packed() is not packed
    b = m.tokenize_ids(img)
    assert not torch.equal(a, b)
    want, safe = tc.judge(tc.encoder64(c1['sd'], c0['img']))
    assert int((~safe).sum()) <= tc.MAX_UNSAFE * safe.numel()
    tc.check_ids(b, want, safe)


# ---- extract_video_tokens and the files ----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_extract_video_tokens(dev):
    from slotformer_amd import harness
    from slotformer_amd.ingest import FrameIngest
    c = tc.model_case(4096, 3, 64, 64)
    m = model_on(dev, c, 4096)
    u8 = torch.randint(0, 256, (3, 5, 64, 64, 3), dtype=torch.uint8, generator=tc.gen(8))
    ing = FrameIngest((64, 64))
    clips = ing(u8.to(dev))                                            # [3, 5, 3, 64, 64] float32: FrameIngest's own output
    want = m.tokenize_ids(clips.flatten(0, 1)).flatten(1, 2).cpu()    # per frame
    for f in (0, 7, 14):
        assert torch.equal(m.tokenize_ids(clips.flatten(0, 1)[f:f + 1]).flatten().cpu(), want[f])
    tok = harness.extract_video_tokens(m, clips, batch_size=2)       # 15 frames in chunks of 2: the last one is ragged
    assert tok.shape == (3, 5, 256) and tok.dtype == torch.int16 and not tok.is_cuda and tok.is_pinned()
    assert torch.equal(tok.long().view(15, 256), want)
    on_dev = harness.extract_video_tokens(m, clips, batch_size=4, to_host=False)
    assert on_dev.is_cuda and on_dev.dtype == torch.int16 and torch.equal(on_dev.cpu(), tok)
    assert torch.equal(harness.extract_video_tokens(m, clips.cpu(), batch_size=64), tok)          # host-resident frames, one chunk
    # raw uint8 clips + ingest=, from the host and from the device
    assert torch.equal(harness.extract_video_tokens(m, u8, batch_size=2, ingest=ing), tok)
    assert torch.equal(harness.extract_video_tokens(m, u8.to(dev), batch_size=7, ingest=ing), tok)
    with pytest.raises(ValueError):
        harness.extract_video_tokens(m, clips, batch_size=2, ingest=ing)                          # floats are no raw frames
    with pytest.raises(ValueError, match='batch_size'):
        harness.extract_video_tokens(m, clips, batch_size=0)


@torch.no_grad()
def test_token_files_feed_steve(dev, tmp_path):
    """tokens extracted, saved, read back as the dataset reads them and fed to STEVE as `token_id` are the targets it trains on"""
    from test_engine_gpu import build
    from slotformer_amd import harness, slot_io
    g = gu.load_golden('steve_tokens')
    m, _ = build(gu.steve_tokens_cfg(), g, 601, dev)
    video = gu.seeded_img(1, 6, 64, seed=603).to(dev)                  # one video of six frames
    tok = harness.extract_video_tokens(m.dvae, video, batch_size=4)
    path = str(tmp_path / 'PhysionTrainMP4s' / 'Drop' / '3.mp4')
    assert slot_io.save_video_tokens([path], tok, 'dvae') == [slot_io.token_path(path, 'dvae')]
    clip = slot_io.read_token_clip(slot_io.token_path(path, 'dvae'), 1, 2, 3)     # frames 1 and 4
    assert clip.dtype == np.int32 and clip.shape == (2, 256)
    assert np.array_equal(clip, tok[0, [1, 4]].numpy())
    m.testing = False
    out = m({'img': video[:, [1, 4]].contiguous(), 'token_id': torch.from_numpy(clip)[None].to(dev)})
    assert out['target_token_id'].dtype == torch.int64 and torch.equal(out['target_token_id'].cpu(), torch.from_numpy(clip).long())
    assert out['pred_token_id'].shape == (2, 256, 64)
