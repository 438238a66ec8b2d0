"""GPU: the soft rows and the sampled ids of the fused token step (`sf_slate_generate_tok_opts_f32`, csrc/slate_step.hip) against float64
restatements built on the kernel's own logits and the host twin of its noise (tests/steve_soft_cases.py), and the render entry points on top.

Measured on one MI355X when this file was written (every test prints its figures; profiles/steve_render_soft.md), bound 1e-3 throughout:
  soft rows against float64, worst over 16 / 1 steps, frames per workgroup 1 / 2 / 4, row_base 0 / 7: 2.1e-6 (v40), 2.4e-6 (v200); the same for
    every frames-per-workgroup; gumbel_softmax_rows + product against the same float64: 1.1e-6 (v40), 1.7e-6 (v200);
  overflow (max |l| * scale = 2341): 1.4e-6;
  images against the float64 decode: soft 1.8e-5 fused, 2.8e-5 unfused, hard 1.5e-5; fused against unfused soft image 2.3e-5;
  sampled tokens: 0 differing from the float64 run at every seed, temperature and frames per workgroup (logits 3.8e-6 .. 4.3e-6);
  chi-square of 4096 draws at V 32: 32.0, 32.7, 29.1 for seeds 31, 32, 33 (bound 61.10).
"""
import functools

import pytest
import torch

import oracle
import steve_soft_cases as sc
from steve_soft_cases import FRAMES, STEPS, rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-3      # the project's bar (test_steve_render_gpu.py)
MULTI = ['v40', 'v200']


def on_device(name, dev):
    c = sc.case(name)
    return c, c['dec'].to(dev), c['slots'].to(dev), c['table'].to(dev).contiguous()


@pytest.mark.parametrize('name', MULTI)
@torch.no_grad()
def test_soft_rows_against_float64(dev, name):
    from slotformer_amd import ops
    c, dec, slots, table = on_device(name, dev)
    V = c['shape'][0]
    worst = 0.
    for steps in (STEPS, 1):
        for fr in (1, 2, 4):
            for row_base in (0, 7):
                tok, lg, rows = dec.generate_tokens(slots, steps, return_logits=True, frames_per_wg=fr, soft_table=table, soft_scale=sc.SOFT_SCALE,
                                                    soft_seed=41, row_base=row_base)
                assert dec.last_generate_form == fr and rows.is_cuda and tuple(rows.shape) == (FRAMES, steps, 64)
                ref = sc.soft_rows64(lg, c['table'], 41, row_base=row_base)
                err = rel_err(rows, ref)
                worst = max(worst, err)
                print(name, 'steps', steps, 'frames_per_wg', fr, 'row_base', row_base, 'soft rows rel_err', err)
                assert bool(torch.isfinite(rows).all()) and err <= RTOL
                # the frames-per-workgroup 0 of a call with an option on is one frame per workgroup
                if fr == 1:
                    tok0, _, rows0 = dec.generate_tokens(slots, steps, return_logits=True, soft_table=table, soft_scale=sc.SOFT_SCALE, soft_seed=41,
                                                         row_base=row_base)
                    assert dec.last_generate_form == 1 and torch.equal(rows0, rows) and torch.equal(tok0, tok)
        # today's route on the same logits and noise (row_base 0: the softmax kernel counts its rows from 0)
        tok, lg = dec.generate_tokens(slots, steps, return_logits=True, frames_per_wg=1)
        unfused = ops.gumbel_softmax_rows(lg, 41, sc.SOFT_SCALE).view(-1, V) @ table
        print(name, 'steps', steps, 'gumbel_softmax_rows + product rel_err', rel_err(unfused.view(FRAMES, steps, 64), sc.soft_rows64(lg, c['table'], 41)))
    print(name, 'soft rows worst rel_err', worst)


@pytest.mark.parametrize('name', MULTI)
@torch.no_grad()
def test_tokens_and_logits_do_not_see_the_soft_rows(dev, name):
    c, dec, slots, table = on_device(name, dev)
    for fr in (1, 2, 4):
        tok, lg = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr)
        tok2, lg2, rows = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr, soft_table=table, soft_seed=42)
        assert torch.equal(tok, tok2) and torch.equal(lg, lg2)
        tok3, none, rows3 = dec.generate_tokens(slots, STEPS, frames_per_wg=fr, soft_table=table, soft_seed=42)   # no logits buffer at all
        assert none is None and torch.equal(tok3, tok) and torch.equal(rows3, rows)
        # sampling changes the tokens, and through them the later logits, but the soft rows still come from the raw logits
        tok4, lg4, rows4 = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr, soft_table=table, soft_seed=42, sample=True,
                                               sample_seed=sc.SAMPLE_SEEDS[0])
        assert not torch.equal(tok4, tok)
        assert rel_err(rows4, sc.soft_rows64(lg4, c['table'], 42)) <= RTOL


@torch.no_grad()
def test_overflow(dev):
    """head weights x 64: (l + g) * 10 goes far past 88, where exp overflows in fp32; the online softmax never forms it"""
    shape, wseed, _ = sc.CASES['v200']
    dec, _ = sc.make_decoder(shape, wseed)
    dec.head.weight.mul_(64.)
    c = sc.case('v200')
    dec, slots, table = dec.to(dev), c['slots'].to(dev), c['table'].to(dev)
    for fr in (1, 2, 4):
        tok, lg, rows = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr, soft_table=table, soft_scale=sc.SOFT_SCALE, soft_seed=43)
        big = float(((lg + 0.).abs().max()) * sc.SOFT_SCALE)
        err = rel_err(rows, sc.soft_rows64(lg, c['table'], 43))
        print('overflow: frames_per_wg', fr, 'max |l| * scale', big, 'soft rows rel_err', err)
        assert big > 3 * 88
        assert bool(torch.isfinite(rows).all()) and err <= RTOL


class _Model:
    """what harness.render_video_slots needs of a model: a device and `render`"""

    def __init__(self, dec, dvae, dev):
        self.dec, self.dvae, self.device = dec, dvae, dev

    def render(self, slots, **kw):
        from slotformer_amd.steve_render import render_slots
        return render_slots(self.dec, self.dvae, slots, **kw)


@functools.lru_cache(maxsize=None)
def image_case():
    """the v200 decoder under the names of a STEVESlotFormer + a dVAE of the same vocabulary over 16 x 16-pixel frames (a 4 x 4 token grid)"""
    shape, wseed, _ = sc.CASES['v200']
    dec, sd = sc.make_decoder(shape, wseed, prefix='decoder.')
    dvae, dsd = sc.make_dvae(shape[0], 914)
    cfg = {'dec_dict': {'dec_num_heads': shape[2], 'dec_num_layers': shape[5]}, 'resolution': (16, 16), 'dvae_dict': {'down_factor': 4}}
    return dec, dvae, sc.double_sd({**sd, **dsd}), cfg, sc.case('v200')['slots']


@torch.no_grad()
def test_chunks_have_the_bits_of_one_call(dev):
    from slotformer_amd import harness
    c, dec, slots, table = on_device('v200', dev)
    kw = dict(frames_per_wg=1, soft_table=table, soft_seed=44, sample=True, temperature=0.5, sample_seed=45)
    tok, _, rows = dec.generate_tokens(slots, STEPS, **kw)
    tok_a, _, rows_a = dec.generate_tokens(slots[:1], STEPS, **kw)
    tok_b, _, rows_b = dec.generate_tokens(slots[1:], STEPS, row_base=1 * STEPS, **kw)
    assert torch.equal(torch.cat([rows_a, rows_b]), rows) and torch.equal(torch.cat([tok_a, tok_b]), tok)
    tok_w, _, rows_w = dec.generate_tokens(slots[1:], STEPS, **kw)     # without the offset the noise is another
    assert not torch.equal(rows_w, rows[1:]) and not torch.equal(tok_w, tok[1:])
    idec, dvae, _, _, islots = image_case()
    idec, dvae, islots = idec.to(dev), dvae.to(dev), islots.to(dev)
    m = _Model(idec, dvae, dev)
    for extra in (dict(), dict(sample=True, temperature=0.5, sample_seed=47)):
        one = m.render(islots, soft=True, fused=True, seed=46, **extra)
        split = [m.render(islots[:1], soft=True, fused=True, seed=46, **extra), m.render(islots[1:], soft=True, fused=True, seed=46, first_frame=1, **extra)]
        for key in ('tokens', 'hard', 'soft'):
            assert torch.equal(torch.cat([s[key] for s in split]), one[key]), key
        video = harness.render_video_slots(m, islots, frames_per_call=2, soft=True, fused=True, seed=46, **extra)
        assert torch.equal(video, one['soft'])
        video = harness.render_video_slots(m, islots, frames_per_call=2, fused=True, seed=46, **extra)
        assert torch.equal(video, one['hard'])
    # one fresh seed serves every chunk of a call: a chunked call is one call with SOME seed, so its frames are finite and of the right shape
    fresh = harness.render_video_slots(m, islots, frames_per_call=2, soft=True, fused=True)
    assert fresh.shape == one['soft'].shape and bool(torch.isfinite(fresh).all())


@torch.no_grad()
def test_images(dev):
    from slotformer_amd import train
    dec, dvae, sd64, cfg, slots = image_case()
    V, P, h = dec.vocab_size, STEPS, 4
    g = train.gumbel_noise(48, FRAMES * P * V).view(FRAMES, P, V).transpose(1, 2).reshape(FRAMES, V, h, h).double()
    soft64, hard64 = oracle.steve_slotformer_decode(slots.double(), sd64, cfg, g)
    dec, dvae, slots = dec.to(dev), dvae.to(dev), slots.to(dev)
    m = _Model(dec, dvae, dev)
    for fr in (0, 1, 2, 4):
        fused = m.render(slots, soft=True, fused=True, seed=48, frames_per_wg=fr)
        assert dec.last_generate_form == (fr or 1)
        e_soft, e_hard = rel_err(fused['soft'], soft64), rel_err(fused['hard'], hard64)
        print('frames_per_wg', fr, 'fused soft image rel_err', e_soft, 'hard', e_hard)
        assert e_soft <= RTOL and e_hard <= RTOL
        plain = m.render(slots, soft=True, seed=48, frames_per_wg=fr)
        e_plain, e_pair = rel_err(plain['soft'], soft64), rel_err(fused['soft'], plain['soft'])
        print('frames_per_wg', fr, 'unfused soft image rel_err', e_plain, 'fused against unfused', e_pair)
        assert torch.equal(fused['tokens'], plain['tokens']) and torch.equal(fused['hard'], plain['hard'])
        assert e_pair <= RTOL
    assert set(m.render(slots, fused=True)) == {'tokens', 'hard'}      # fused without soft: nothing to fuse


@pytest.mark.parametrize('name', MULTI)
@torch.no_grad()
def test_sampled_tokens_equal_the_float64_run(dev, name):
    """Premise (tests/test_steve_soft_render.py): no position of the float64 run is a near tie for these seeds and temperatures."""
    c, dec, slots, table = on_device(name, dev)
    for seed in sc.SAMPLE_SEEDS:
        for T in sc.TEMPERATURES:
            idx, logits, margin = sc.sampled_run64(name, seed, T)
            assert margin > 1e-4
            for fr in (0, 1, 2, 4):
                tok, lg = dec.generate_tokens(slots, STEPS, return_logits=True, frames_per_wg=fr, sample=True, temperature=T, sample_seed=seed)
                assert dec.last_generate_form == (fr or 1)
                print(name, 'seed', seed, 'T', T, 'frames_per_wg', fr, 'tokens differing', int((tok.cpu() != idx).sum()), 'logits rel_err',
                      rel_err(lg, logits))
                assert torch.equal(tok.cpu(), idx) and rel_err(lg, logits) < 5e-5
                again, none = dec.generate_tokens(slots, STEPS, frames_per_wg=fr, sample=True, temperature=T, sample_seed=seed)
                assert none is None and torch.equal(again, tok)
            tok_g, lg_g = dec.generate(slots, STEPS, sample=True, temperature=T, seed=seed)
            assert tok_g.is_cuda and not lg_g.is_cuda and torch.equal(tok_g, tok) and torch.equal(lg_g, lg.cpu())
    # one step, with an offset: the BOS-only path
    idx, _, _ = sc.sampled_run64(name, sc.SAMPLE_SEEDS[0], 1.0, steps=1, row_base=7)
    tok, _ = dec.generate_tokens(slots, 1, sample=True, sample_seed=sc.SAMPLE_SEEDS[0], row_base=7)
    assert torch.equal(tok.cpu(), idx)


@pytest.mark.parametrize('seed', sc.CHI2_SEEDS)
@torch.no_grad()
def test_draw_statistics(dev, seed):
    from slotformer_amd import train
    c, dec, slots, _ = on_device('v32', dev)
    same = slots[:1].expand(sc.DRAWS, -1, -1).contiguous()
    tok, lg = dec.generate_tokens(same, 1, return_logits=True, sample=True, sample_seed=seed)
    assert dec.last_generate_form == 1 and bool((lg == lg[:1]).all())
    p = torch.softmax(lg[0, 0].cpu().double(), 0)
    chi2 = sc.chi_square(torch.bincount(tok.flatten().cpu(), minlength=32), p)
    print('seed', seed, 'chi-square of', sc.DRAWS, 'draws', chi2, 'smallest expected count', float(p.min()) * sc.DRAWS)
    assert chi2 < sc.CHI2_31_999
    # and they are the twin's draws, wherever the float64 score has no near tie (fp32 rounds the score at 6e-8 of its size)
    score = lg[:, 0].cpu().double() + train.gumbel_noise(seed, sc.DRAWS * 32).view(sc.DRAWS, 32).double()
    top2 = score.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5 * score.abs().max()
    assert int(clear.sum()) > sc.DRAWS - 8 and torch.equal(tok.flatten().cpu()[clear], score.argmax(-1)[clear])


@torch.no_grad()
def test_what_is_not_asked_for_does_not_change(dev):
    from slotformer_amd import harness, ops
    c, dec, slots, _ = on_device('v40', dev)
    dec.last_generate_form = 'untouched'
    torch.manual_seed(7)
    a, la = dec.generate(slots, 4, sample=True, temperature=0.7)
    torch.manual_seed(7)
    b, lb = dec.generate(slots, 4, sample=True, temperature=0.7)
    assert dec.last_generate_form == 'untouched' and torch.equal(a, b) and torch.equal(la, lb) and not la.is_cuda     # torch.multinomial, prefix re-run
    idec, dvae, _, _, islots = image_case()
    idec, dvae, islots = idec.to(dev), dvae.to(dev), islots.to(dev)
    m = _Model(idec, dvae, dev)
    old = m.render(islots, soft=True, seed=49)
    new = m.render(islots, soft=True, seed=49, fused=False, first_frame=0, sample=False, temperature=1.0, sample_seed=None)
    tok, lg = idec.generate_tokens(islots, STEPS, return_logits=True)                                    # the route as it was, restated
    z = ops.gumbel_softmax_rows(lg, 49, 10.0).view(FRAMES, 4, 4, idec.vocab_size)
    soft = torch.cat([dvae.detokenize_nhwc(z[i:i + 1]) for i in range(FRAMES)])
    for key in ('tokens', 'hard', 'soft'):
        assert torch.equal(old[key], new[key])
    assert torch.equal(old['soft'], soft) and torch.equal(old['tokens'].flatten(1), tok)
    assert torch.equal(harness.render_video_slots(m, islots, frames_per_call=2), old['hard'])
    assert torch.equal(harness.render_video_slots(m, islots, frames_per_call=2, fused=False, seed=None, sample=False, temperature=1.0, sample_seed=None),
                       old['hard'])
    # detokenize_ids through detokenize_rows: the bits of the gather + GroupNorm + tail it was
    ids = old['tokens']
    blk = dvae.decoder[0]
    y = ops.gather_rows(dvae.conv0_table(), ids.contiguous())
    tail = dvae._decoder_tail(ops.groupnorm1_nhwc(y, blk.weight.detach(), blk.bias.detach(), relu=True))
    assert torch.equal(dvae.detokenize_ids(ids), tail) and torch.equal(dvae.detokenize_rows(y), tail)
