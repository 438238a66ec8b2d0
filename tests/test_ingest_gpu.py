"""GPU: the ingest kernels (csrc/ingest.hip) against torch on the CPU in float64, and the `ingest=` path of the pipeline / the harness against the
same calls on the float32 frames the ingest produced beforehand.

The bound: |kernel - float64| <= 4e-6 absolute on outputs in [-1, 1].  With float64-built tables the only errors are the float32 rounding of each
weight, of each product and of the running sums, and of the final normalisation: at most a few dozen roundings of 2^-24 on values <= 1 for up to a
15 x 15-tap footprint.  A case beyond it means wrong tables or wrong clamping."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import ingest_cases as ic

pytestmark = pytest.mark.gpu


def _err(got, ref):
    return (got.cpu().double() - ref).abs().max().item()


@pytest.mark.parametrize('antialias', [False, True])
@pytest.mark.parametrize('src,dst', ic.SHAPES)
def test_frames_kernel_matches_float64(dev, src, dst, antialias):
    from slotformer_amd.ingest import FrameIngest
    u8 = ic.frames_of(*src)
    ref = ic.reference_of(*src, *dst, int(antialias))
    ing = FrameIngest(dst, antialias=antialias)
    got = ing.ingest(u8.to(dev))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(ref.shape)
    e = _err(got, ref)
    print(f'kernel {src}->{dst} aa={antialias}: max err {e:.2e}')
    assert e <= ic.BOUND
    # a capped grid (the workgroups loop over the bands) computes the same bits; so does a [B, T, ...] clip into out=
    ing.max_blocks = 3
    assert torch.equal(ing.ingest(u8.to(dev)), got)
    ing.max_blocks = 0
    out = torch.full((1, ic.NFRAMES, 3) + tuple(dst), 7., device=dev)
    assert ing(u8.to(dev)[None], out=out) is out and torch.equal(out[0], got)
    # the plain-torch path on the CPU applies the same tables
    assert _err(got, ing.ingest(u8).double()) <= 2 * ic.BOUND


@pytest.mark.parametrize('antialias', [False, True])
def test_palette_kernel(dev, antialias):
    from slotformer_amd.ingest import FrameIngest
    idx, pal, rgb = ic.palette_case()
    _, dst = ic.PALETTE_SHAPE
    ref = ic.yardstick(rgb, dst, antialias)
    got = FrameIngest(dst, antialias=antialias, palette=pal).ingest(idx.to(dev))
    e = _err(got, ref)
    print(f'palette aa={antialias}: max err {e:.2e}')
    assert e <= ic.BOUND


@pytest.mark.parametrize('antialias', [False, True])
@pytest.mark.parametrize('offset', [1, 3, 7])
def test_misaligned_source_and_channel_statistics(dev, offset, antialias):
    """The first case again with the source a view at a byte offset into a larger buffer, and per-channel mean / std."""
    from slotformer_amd.ingest import FrameIngest
    (H0, W0), dst = ic.SHAPES[0]
    u8 = ic.frames_of(H0, W0)
    mean, std = (0.4, 0.5, 0.6), (0.6, 0.5, 0.7)      # (outputs stay within [-1, 1])
    ref = ic.yardstick(u8, dst, antialias, mean, std)
    assert ref.abs().max() <= 1.0
    big = torch.full((u8.numel() + 64, ), 255, dtype=torch.uint8, device=dev)
    view = big[offset:offset + u8.numel()].view(u8.shape)
    view.copy_(u8.to(dev))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    got = FrameIngest(dst, mean=mean, std=std, antialias=antialias).ingest(view)
    e = _err(got, ref)
    print(f'offset {offset} aa={antialias}: max err {e:.2e}')
    assert e <= ic.BOUND
    # an output that is not 16-byte aligned takes the scalar stores
    obuf = torch.empty(ref.numel() + 4, device=dev)
    out = obuf[1:1 + ref.numel()].view(ref.shape)
    FrameIngest(dst, mean=mean, std=std, antialias=antialias).ingest(view, out=out)
    assert torch.equal(out, got)


@pytest.mark.parametrize('src,dst', [((320, 480), (128, 128)), ((5, 7), (64, 64)), ((29, 37), (29, 37))])
def test_mask_kernel_is_interpolate_nearest(dev, src, dst):
    from slotformer_amd.ingest import FrameIngest
    rs = np.random.RandomState(9)
    m = torch.from_numpy(rs.randint(0, 256, size=(ic.NFRAMES, ) + src)).long()    # ids up to 255
    ref = F.interpolate(m[None].double(), dst, mode='nearest')[0].long()
    ing = FrameIngest(dst)
    for din in (torch.int64, torch.uint8):
        for dout in (torch.int64, torch.uint8):
            got = ing.process_mask(m.to(din).to(dev), dtype=dout)
            assert got.dtype == dout and got.is_cuda and torch.equal(got.cpu().long(), ref), (din, dout)
    assert torch.equal(ing.process_mask(m[0].to(dev)).cpu(), ref[0])     # [H0, W0]
    assert torch.equal(ing.process_mask(m).long(), ref)                  # the CPU path picks the same pixels


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------------
def _res64_models(dev):
    from slotformer_amd.base_slots import build_model
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(21)
    savi = build_model(gu.ParamsView(gu.savi_cfg(64, 7, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'))).eval().to(dev)
    savi.testing = True
    roll = SlotRollouter(**gu.C2_ROLL['rollout_dict']).eval().to(dev)
    return savi, roll


@torch.no_grad()
def test_extract_and_rollout_with_ingest(dev):
    """Raw uint8 50 x 70 clips through extract_and_rollout(ingest=...) -- pinned, pageable and device input, pipelined and serial, more full batches
    than the staging ring has slots plus a ragged tail, different content in every batch -- must be torch.equal to extract_and_rollout on the float32
    frames ingest(frames) produced beforehand: both sides run the same encode and rollout kernels on the same bits, so any difference is a stale or
    raced staging slot."""
    from slotformer_amd import harness
    from slotformer_amd.ingest import FrameIngest
    savi, roll = _res64_models(dev)
    B, T, H, G = 3, 6, 4, 2
    ring = 4 * G + G + 2                      # (checked against the pipeline object below)
    V = B * (ring + 3) + 1                    # more full batches than ring slots + a ragged tail
    rs = np.random.RandomState(13)
    clips = torch.from_numpy(rs.randint(0, 256, size=(V, T, 50, 70, 3), dtype=np.uint8))
    noises = torch.from_numpy(rs.standard_normal((V, T, 7, 128)).astype(np.float32))
    ing = FrameIngest((64, 64))
    try:
        frames = ing.ingest(clips.to(dev))                     # [V, T, 3, 64, 64] float32, beforehand
        assert _err(frames[:2].flatten(0, 1), ic.yardstick(clips[:2].flatten(0, 1), (64, 64), False)) <= ic.BOUND
        ref = harness.extract_and_rollout(savi, roll, frames, H, batch_size=B, noises=noises, group=G)
        pipe = next(iter(harness._PIPES.values()))[2]
        assert pipe.stage_slots == ring and V // B > pipe.stage_slots
        inputs = {'pinned': clips.pin_memory(), 'pageable': clips, 'device': clips.to(dev)}
        for name, vid in inputs.items():
            for pipelined in (True, False):
                out = harness.extract_and_rollout(savi, roll, vid, H, batch_size=B, noises=noises, pipelined=pipelined, ingest=ing, group=G)
                assert torch.equal(out, ref), (name, pipelined)
        # the float32 path of the same pipeline object is unchanged by the uint8 runs in between (host input: its own staging ring)
        assert torch.equal(harness.extract_and_rollout(savi, roll, frames.cpu(), H, batch_size=B, noises=noises, group=G), ref)
        out_h = harness.extract_and_rollout(savi, roll, inputs['pinned'], H, batch_size=B, noises=noises, to_host=True, ingest=ing, group=G)
        assert not out_h.is_cuda and torch.equal(out_h, ref.cpu())
        # with ingest= anything but uint8 raises (no silent 0..255 floats); without it the float32 check stands
        with pytest.raises(ValueError, match='uint8'):
            harness.extract_and_rollout(savi, roll, frames, H, batch_size=B, noises=noises, ingest=ing, group=G)
        with pytest.raises(ValueError, match='uint8'):
            pipe.run([frames[:B]], ingest=ing)
        with pytest.raises(RuntimeError, match='float32'):
            pipe.run([clips[:B].to(dev)])
    finally:
        harness.release_pipelines()


@torch.no_grad()
def test_extract_and_rollout_with_ingest_and_decoder(dev):
    from slotformer_amd import harness
    from slotformer_amd.ingest import FrameIngest
    savi, roll = _res64_models(dev)
    B, T, H, V = 3, 6, 4, 3 * 4 + 2
    rs = np.random.RandomState(14)
    clips = torch.from_numpy(rs.randint(0, 256, size=(V, T, 50, 70, 3), dtype=np.uint8))
    noises = torch.from_numpy(rs.standard_normal((V, T, 7, 128)).astype(np.float32))
    ing = FrameIngest((64, 64), antialias=True)
    try:
        frames = ing.ingest(clips.to(dev))
        ref, rdec = harness.extract_and_rollout(savi, roll, frames, H, batch_size=B, noises=noises, decoder=savi)
        out, dec = harness.extract_and_rollout(savi, roll, clips.pin_memory(), H, batch_size=B, noises=noises, decoder=savi, ingest=ing)
        assert torch.equal(out, ref) and torch.equal(dec['recon'], rdec['recon']) and torch.equal(dec['seg'], rdec['seg'])
    finally:
        harness.release_pipelines()
