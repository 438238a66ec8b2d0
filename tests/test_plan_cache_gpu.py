"""Plan-cache invalidation: derived / packed weight copies are keyed on (data_ptr, _version) of the parameters.
FlatAdam writes the parameters through a raw pointer and must bump the versions; modules must stay copyable / picklable after
a forward (the plans hold ctypes structures with raw pointers)."""
import copy
import io

import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu


def _slotformer(dev, seed=0):
    from test_engine_gpu import build
    m, _ = build(gu.C2_ROLL, gu.load_golden('roll_c2'), 202 + seed, dev, vp=True)
    return m


def test_flat_adam_invalidates_inference_plans(dev):
    """eval -> FlatAdam steps -> eval must equal a FRESHLY constructed model holding the stepped weights (the fused d=256
    rollout path serves fragment-ordered copies of every weight)."""
    from slotformer_amd import train
    cfg = gu.C2_ROLL
    rd = cfg['rollout_dict']
    m = _slotformer(dev)
    x = gu.seeded_normal((2, rd['history_len'], rd['num_slots'], rd['slot_size']), 3).to(dev)
    m.eval()
    with torch.no_grad():
        before = m.rollouter(x, 4).clone()              # builds the packed inference plan
    opt = train.FlatAdam([p for p in m.rollouter.parameters() if p.requires_grad], lr=1e-2)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.
    slots = gu.seeded_normal((2, rd['history_len'] + 3, rd['num_slots'], rd['slot_size']), 4).to(dev)
    m.rollout_len = 3
    for _ in range(3):
        opt.zero_grad()
        out = m({'slots': slots})
        m.calc_train_loss({'slots': slots}, out)['slot_recon_loss'].backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        after = m.rollouter(x, 4).clone()
    assert not torch.equal(before, after), 'the optimizer steps did not reach the inference path (stale packed weights)'
    fresh = _slotformer(dev, seed=1)
    fresh.load_state_dict(m.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh.rollouter(x, 4)
    assert torch.equal(after, want), (after - want).abs().max().item()


def test_invalidate_after_data_write(dev):
    from slotformer_amd import engine
    m = _slotformer(dev).eval()
    rd = gu.C2_ROLL['rollout_dict']
    x = gu.seeded_normal((2, rd['history_len'], rd['num_slots'], rd['slot_size']), 3).to(dev)
    with torch.no_grad():
        a = m.rollouter(x, 3).clone()
        m.rollouter.out_proj.weight.data.mul_(0.5)        # bypasses torch's version counter
        engine.invalidate(m)
        b = m.rollouter(x, 3).clone()
    assert not torch.equal(a, b)


def test_modules_stay_copyable_and_picklable_after_forward(dev):
    m = _slotformer(dev).eval()
    rd = gu.C2_ROLL['rollout_dict']
    x = gu.seeded_normal((1, rd['history_len'], rd['num_slots'], rd['slot_size']), 3).to(dev)
    with torch.no_grad():
        a = m.rollouter(x, 2)
        m2 = copy.deepcopy(m)                             # EMA copies, STEVESlotFormer's decoder copy
        assert torch.equal(m2.rollouter(x, 2), a)
        buf = io.BytesIO()
        torch.save(m, buf)                                # whole-module pickling
        buf.seek(0)
        m3 = torch.load(buf, weights_only=False)
        assert torch.equal(m3.rollouter(x, 2), a)


def _small_decoder(dev):
    """decoder 'small' of test_steve_render_gpu.py with 2 frames of slots (a fresh module: the tests below write its weights)"""
    from test_steve_render_gpu import make_decoder, CASES
    shape, wseed, sseed = CASES['small']
    dec, _ = make_decoder(shape, wseed)
    return dec.to(dev), gu.seeded_normal((2, shape[4], shape[1]), sseed).to(dev)


@torch.no_grad()
def test_decoder_copy_builds_its_own_slate_plan(dev):
    """`copy.deepcopy` of a decoder that has generated once (its slate plan holds ctypes pointers) raised ValueError before the plans
    lived in the one cache that copies as empty.  The copy serves its own weights: a write to the original does not reach it."""
    from slotformer_amd import engine
    dec, slots = _small_decoder(dev)
    tok, lg = dec.generate_cached(slots, 8)
    twin = copy.deepcopy(dec)
    tok2, lg2 = twin.generate_cached(slots, 8)
    assert torch.equal(tok2, tok) and torch.equal(lg2, lg)
    dec.head.weight.data.mul_(0.5)                        # bypasses torch's version counter
    engine.invalidate(dec)
    assert not torch.equal(dec.generate_cached(slots, 8)[1], lg)
    tok3, lg3 = twin.generate_cached(slots, 8)
    assert torch.equal(tok3, tok) and torch.equal(lg3, lg)


@torch.no_grad()
def test_decoder_forward_after_invalidate(dev):
    """`forward` reads its concatenated projections through the cache `invalidate` empties (it raised AttributeError after `invalidate`
    while that cache was an attribute only the constructor created): untouched weights, equal bits."""
    from slotformer_amd import engine
    dec, slots = _small_decoder(dev)
    idx = (torch.arange(2 * 7).view(2, 7) * 11 % dec.vocab_size).to(dev)
    a = dec(slots, idx).clone()
    engine.invalidate(dec)
    assert torch.equal(dec(slots, idx), a)


@torch.no_grad()
def test_dvae_invalidate_after_data_write(dev):
    """The dVAE's derived copies (the transposed first decoder weight `detokenize_ids` gathers from, the OHWI copies of the 3x3 weights) are
    rebuilt after `invalidate`; a `.data` write alone bypasses the version counter and keeps them, which is the documented contract.
    (Halving a weight in front of GroupNorm changes the output through the norm's eps: 5e-4 relative at these weights, far above rounding.)"""
    from slotformer_amd import engine
    from slotformer_amd.base_slots.models.dVAE import dVAE
    torch.manual_seed(7)
    m = dVAE(64).to(dev).eval()
    ids = (torch.arange(16).view(1, 4, 4) * 5 % 64).to(dev)
    for blk in (m.decoder[0], m.decoder[1]):              # the gathered table; a 3x3 block
        a = m.detokenize_ids(ids).clone()
        blk.m.weight.data.mul_(0.5)
        assert torch.equal(m.detokenize_ids(ids), a)
        engine.invalidate(m)
        assert not torch.equal(m.detokenize_ids(ids), a)
