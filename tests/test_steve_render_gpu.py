"""GPU: STEVE slots -> frames on the device.  The one-launch token step (`sf_slate_generate_tok_f32`, csrc/slate_step.hip) against the float64 oracle
and against the launch chain it replaces; the gather detokeniser; `render` / `render_video_slots` / `make_steve_video` against the committed fixtures
and plain-torch restatements."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-3      # north-star bar of the golden fixtures (test_engine_gpu.py)
STEPS, FRAMES = 136, 5   # 136 steps cross the 64- and 128-key marks of a key tiling; 5 frames leave a ragged last workgroup at 2 and 4 frames per workgroup

CASES = {
    # name: ((V, d, heads, max_len, slots, blocks), weights seed, slots seed)
    'physion': ((4096, 192, 4, 1023, 6, 4), 901, 1901),   # head size 48: not a power of two
    'small': ((64, 64, 4, 255, 4, 2), 902, 1902),
}


def rel_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max()).item()


def make_decoder(shape, seed):
    """(module on the CPU in eval mode, state dict under the oracle's 'trans_decoder.' names)"""
    from slotformer_amd.base_slots.models.steve_transformer import STEVETransformerDecoder
    dec = STEVETransformerDecoder(*shape)
    own = {'trans_decoder.' + k: v for k, v in dec.state_dict().items()}
    sd = gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in own.items()], seed, keep=own)
    dec.load_state_dict({k[len('trans_decoder.'):]: v for k, v in sd.items()}, strict=True)
    return dec.eval(), sd


@functools.lru_cache(maxsize=None)
def case(name):
    """decoder, slots and the float64 oracle's greedy run (computed once per process, never modified)"""
    shape, wseed, sseed = CASES[name]
    dec, sd = make_decoder(shape, wseed)
    slots = gu.seeded_normal((FRAMES, shape[4], shape[1]), sseed)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        idx, logits = oracle.steve_decoder_generate(slots.double(), STEPS, sd64, shape[2], shape[5])
    top2 = logits.topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1]) / logits.abs().max()
    return dict(dec=dec, slots=slots, idx=idx, logits=logits, margin=margin, shape=shape)


@pytest.mark.parametrize('name', ['physion', 'small'])
@torch.no_grad()
def test_tokens_and_logits_against_float64(dev, name):
    """Premise (checked on the CPU when this test was written): the oracle's own greedy run has a smallest top-2 margin of 2.67e-4 (physion) and
    1.81e-4 (small) of max|logit|, so no position is a near tie and the fp32 tokens must EQUAL the float64 ones."""
    c = case(name)
    print(name, 'smallest top-2 margin / max|logit|', float(c['margin'].min()))
    assert float(c['margin'].min()) > 1e-4          # the `safe` rule of test_engine_gpu.py, on every position
    dec = c['dec'].to(dev)
    slots = c['slots'].to(dev)
    for fr in (0, 1, 2, 4):
        tok, lg = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr)
        form = dec.last_generate_form
        err = rel_err(lg, c['logits'])
        print(name, 'frames_per_wg', fr, 'ran', form, 'logits rel_err', err, 'tokens differing', int((tok.cpu() != c['idx']).sum()))
        assert tok.is_cuda and lg.is_cuda and tok.dtype == torch.int64 and tuple(lg.shape) == (FRAMES, STEPS, c['shape'][0])
        assert torch.equal(tok.cpu(), c['idx'])
        assert err < 5e-5
        tok2, none = dec.generate_tokens(slots, STEPS, frames_per_wg=fr)
        assert none is None and torch.equal(tok2, tok)
        assert form == (fr if fr else form) and form in (1, 2, 4)      # the fused step is the form that ran


@torch.no_grad()
def test_fused_step_equals_the_launch_chain(dev):
    c = case('physion')
    dec = c['dec'].to(dev)
    slots = c['slots'].to(dev)
    t_chain, l_chain = dec.generate_cached(slots, STEPS)
    tok, lg = dec.generate_tokens(slots, STEPS, return_logits=True)
    err = rel_err(lg, l_chain)
    print('fused vs chain: logits rel_err', err)
    assert torch.equal(tok, t_chain) and err < 1e-5     # the bound the cached and prefix-rerun forms are held to (test_engine_gpu.py)


@torch.no_grad()
def test_one_frame_and_one_step(dev):
    """the degenerate grid (B = 1) and the BOS-only path (steps = 1)"""
    c = case('small')
    dec = c['dec'].to(dev)
    slots = c['slots'].to(dev)
    for fr in (0, 1, 2, 4):
        tok, lg = dec.generate_tokens(slots[:1], 1, return_logits=True, frames_per_wg=fr)
        assert dec.last_generate_form in (1, 2, 4)
        assert torch.equal(tok.cpu(), c['idx'][:1, :1]) and rel_err(lg, c['logits'][:1, :1]) < 5e-5
        tok, lg = dec.generate_tokens(slots[:1], STEPS, return_logits=True, frames_per_wg=fr)     # one frame, every step
        assert torch.equal(tok.cpu(), c['idx'][:1]) and rel_err(lg, c['logits'][:1]) < 5e-5
        tok, lg = dec.generate_tokens(slots, 1, return_logits=True, frames_per_wg=fr)             # every frame, one step
        assert torch.equal(tok.cpu(), c['idx'][:, :1]) and rel_err(lg, c['logits'][:, :1]) < 5e-5


@torch.no_grad()
def test_fallback_to_the_launch_chain(dev):
    """A decoder that sf_slate_step_ok refuses because d_model % 32 != 0: generate_tokens runs the launch chain, says so, and leaves the logits on
    the device.  The width is 48 (3 heads of 16), not 40: the launch chain itself takes head sizes 16, 32, 48 and 64 only, which no head count
    gives at d_model 40, so a decoder of that width cannot be generated from by either form (that sf_slate_step_ok refuses 40 / 4 heads is checked on
    the CPU, tests/test_steve_render.py)."""
    import ctypes as C
    from slotformer_amd import _lib
    dec, _ = make_decoder((32, 48, 3, 31, 3, 2), 903)
    dec = dec.to(dev)
    assert _lib.lib().sf_slate_step_ok(C.byref(dec._slate_plan().struct)) == 0
    slots = gu.seeded_normal((3, 3, 48), 1903).to(dev)
    t_chain, l_chain = dec.generate_cached(slots, 20)
    for fr in (0, 2):
        tok, lg = dec.generate_tokens(slots, 20, return_logits=True, frames_per_wg=fr)
        assert dec.last_generate_form == 0
        assert lg.is_cuda and torch.equal(tok, t_chain) and rel_err(lg, l_chain) < 1e-5


@torch.no_grad()
def test_detokenize_ids(dev):
    from test_engine_gpu import build
    g = gu.load_golden('steve_tokens')
    m, _ = build(gu.steve_tokens_cfg(), g, 601, dev)
    ids = torch.from_numpy(g['dvae_ids']).to(dev)
    z_hard = torch.zeros(2, 64, 16, 16).scatter_(1, torch.from_numpy(g['dvae_ids']).unsqueeze(1), 1.).to(dev)
    got = m.dvae.detokenize_ids(ids)
    assert got.is_cuda and tuple(got.shape) == (2, 3, 64, 64)
    assert rel_err(got, m.dvae.detokenize(z_hard).cpu()) < 1e-4
    assert rel_err(got, g['recon_hard']) < 1e-4
    assert rel_err(m.dvae.detokenize_nhwc(z_hard.permute(0, 2, 3, 1)), m.dvae.detokenize(z_hard).cpu()) < 1e-6


def steve_slotformer(dev, tmp_path):
    """the model of test_steve_slotformer_golden, built exactly as that test builds it"""
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    g = gu.load_golden('steve_slotformer')
    steve = bb(gu.ParamsView(gu.steve_tokens_cfg()))
    path = str(tmp_path / 'steve.pth')
    torch.save({'state_dict': steve.state_dict()}, path)
    cfg = gu.steve_slotformer_cfg()
    cfg['dec_dict']['dec_ckp_path'] = path
    m = bv(gu.ParamsView(cfg))
    shapes = gu.shapes_from_golden(g)
    own = dict(m.state_dict())
    assert [(k, tuple(v.shape)) for k, v in own.items()] == shapes
    sd = gu.seeded_state_dict(shapes, 701, keep=own)
    m.load_state_dict(sd, strict=True)
    return m.eval().to(dev), g, sd, cfg


@torch.no_grad()
def test_steve_slotformer_render(dev, tmp_path):
    m, g, sd, cfg = steve_slotformer(dev, tmp_path)
    slots = torch.from_numpy(g['pred_slots'][:, 0]).to(dev)
    gumbel = torch.from_numpy(g['gumbel'])
    out = m.render(slots, soft=True, gumbel=gumbel)
    assert all(v.is_cuda for v in out.values()) and out['tokens'].dtype == torch.int64
    print('render soft', rel_err(out['soft'], g['soft_recon']), 'hard', rel_err(out['hard'], g['hard_recon']))
    assert rel_err(out['hard'], g['hard_recon']) < RTOL
    assert rel_err(out['soft'], g['soft_recon']) < 5 * RTOL
    # the tokens are the argmax of decode's path (the launch chain's logits)
    _, l_chain = m.decoder.generate_cached(slots, m.num_patches)
    assert torch.equal(out['tokens'].flatten(1).cpu(), l_chain.argmax(-1))
    hard_only = m.render(slots)
    assert set(hard_only) == {'tokens', 'hard'} and torch.equal(hard_only['hard'], out['hard']) and torch.equal(hard_only['tokens'], out['tokens'])
    # noise generated in the kernel: a pure function of the seed
    a, b, c = (m.render(slots, soft=True, seed=s)['soft'] for s in (11, 11, 12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    fresh = m.render(slots, soft=True)['soft']
    assert all(bool(torch.isfinite(t).all()) for t in (a, c, fresh, out['soft'], out['hard'])) and fresh.shape == a.shape


@torch.no_grad()
def test_render_video_slots_and_steve_video(dev, tmp_path):
    from slotformer_amd import egress, harness
    from slotformer_amd.video_prediction import vp_vis
    m, g, sd, cfg = steve_slotformer(dev, tmp_path)
    rd = cfg['rollout_dict']
    slots = gu.seeded_normal((2, 3, rd['num_slots'], rd['slot_size']), 704).to(dev)
    whole = m.render(slots.flatten(0, 1))['hard']
    video = harness.render_video_slots(m, slots, frames_per_call=4)                  # 6 frames: chunks of 4 and 2
    assert video.is_cuda and tuple(video.shape) == (2, 3, 3, 64, 64) and torch.equal(video.flatten(0, 1), whole)
    assert torch.equal(harness.render_video_slots(m, slots[0], frames_per_call=2), video[0])
    u8 = harness.render_video_slots(m, slots, frames_per_call=4, to_host=True)
    assert not u8.is_cuda and u8.is_pinned() and u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 3, 64, 64, 3)
    assert torch.equal(u8, egress.frames_to_uint8(video).cpu())
    # the three-tile video against a plain-torch restatement of make_grid(nrow=3, padding=2) over to_rgb of the stack
    gt = gu.seeded_img(1, 3, 64, seed=705)[0].to(dev)
    soft = m.render(slots[0], soft=True, seed=5)['soft']
    tiles = (torch.stack([gt, soft, video[0]], 1).cpu() * 0.5 + 0.5).clamp(0, 1)     # [T, 3 tiles, 3, H, W]
    ref = torch.zeros(3, 3, 64 + 4, 3 * 66 + 2)
    for k in range(3):
        ref[:, :, 2:66, k * 66 + 2:k * 66 + 66] = tiles[:, k]
    got = vp_vis.make_steve_video(gt, soft, video[0])
    assert got.is_cuda and torch.equal(got.cpu(), ref)
    got8 = vp_vis.make_steve_video_u8(gt, soft, video[0])
    assert got8.is_cuda and got8.dtype == torch.uint8 and torch.equal(got8.cpu(), (ref * 255.).to(torch.uint8).permute(0, 2, 3, 1))
    assert torch.equal(vp_vis.make_steve_video_u8(gt, soft, video[0], layout='chw').cpu(), (ref * 255.).to(torch.uint8))
