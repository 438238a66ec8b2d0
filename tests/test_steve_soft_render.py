"""CPU: what of the soft rows / sampled ids of the fused token step (`sf_slate_generate_tok_opts_f32`, csrc/slate_step.hip) can be checked
without a GPU -- the ABI, the argument errors (all reported before any device work), the host twin of the noise at an offset, the distribution
of Gumbel-max on that twin, and the premise of the GPU test that demands sampled tokens EQUAL to the float64 run (no near tie)."""
import ctypes as C
import math

import pytest
import torch

import steve_soft_cases as sc
from slotformer_amd import _lib, train
from test_steve_render import desc


def opts(**kw):
    o = _lib.sf_slate_step_opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def call(o, m=None, B=1, steps=1):
    one = C.c_void_p(16)   # a non-null dummy pointer, never dereferenced: every call below must fail before any device work
    m = desc() if m is None else m
    return _lib.lib().sf_slate_generate_tok_opts_f32(C.byref(m), one, B, steps, one, None, 0, one, 1 << 40, None, None,
                                                     None if o is None else C.byref(o))


def test_symbols_and_struct():
    lib = _lib.lib()
    assert hasattr(lib, 'sf_slate_generate_tok_opts_f32') and hasattr(lib, 'sf_slate_generate_tok_opts_workspace_bytes')
    o = _lib.sf_slate_step_opts
    # include/slotformer_hip.h: two pointers, int, float, uint64, int, float, uint64, int64
    assert C.sizeof(o) == 2 * 8 + 2 * 4 + 8 + 2 * 4 + 8 + 8 == 56
    assert [getattr(o, n).offset for n in ('soft_rows', 'conv0_t', 'conv0_width', 'soft_scale', 'soft_seed', 'sample', 'inv_temperature',
                                           'sample_seed', 'row_base')] == [0, 8, 16, 20, 24, 32, 36, 40, 48]
    m = desc()
    soft = opts(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=10.)
    ws = lib.sf_slate_generate_tok_opts_workspace_bytes
    for B, steps in ((1, 1), (12, 1024), (5, 16), (64, 1024)):
        plain = lib.sf_slate_generate_tok_workspace_bytes(C.byref(m), B, steps)
        assert ws(C.byref(m), B, steps, None) == ws(C.byref(m), B, steps, C.byref(opts())) == plain > 0     # no option: the plain query
        # an option on: the fused step's scratch alone -- no more than either form's, and no term in the vocabulary
        assert 0 < ws(C.byref(m), B, steps, C.byref(soft)) == ws(C.byref(m), B, steps, C.byref(opts(sample=1, inv_temperature=1.))) <= plain
        assert ws(C.byref(desc(vocab=8192)), B, steps, C.byref(soft)) == ws(C.byref(m), B, steps, C.byref(soft))
    assert ws(C.byref(m), 0, 4, C.byref(soft)) == 0 and ws(None, 4, 4, C.byref(soft)) == 0
    small = desc(d=48, heads=3)     # refused by the fused step: the plain query's value, and the call itself is an error
    assert ws(C.byref(small), 3, 8, C.byref(soft)) == lib.sf_slate_generate_tok_workspace_bytes(C.byref(small), 3, 8)


@pytest.mark.parametrize('kw, word', [
    (dict(soft_rows=16, conv0_t=None, conv0_width=64, soft_scale=10.), b'conv0_t'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=32, soft_scale=10.), b'conv0_width'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=128, soft_scale=10.), b'conv0_width'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=0.), b'soft_scale'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=-1.), b'soft_scale'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=math.inf), b'soft_scale'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=math.nan), b'soft_scale'),
    (dict(sample=1, inv_temperature=0.), b'inv_temperature'),
    (dict(sample=1, inv_temperature=-2.), b'inv_temperature'),
    (dict(sample=1, inv_temperature=math.inf), b'inv_temperature'),
    (dict(sample=1, inv_temperature=math.nan), b'inv_temperature'),
    (dict(sample=1, inv_temperature=1., row_base=-1), b'row_base'),
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=10., row_base=-7), b'row_base'),
    (dict(sample=1, inv_temperature=1., row_base=(1 << 20) - 1), b'2^32'),     # (2^20 - 1 + 1 * 1) * 4096 = 2^32
    (dict(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=10., row_base=1 << 40), b'2^32'),
])
def test_argument_errors_come_before_any_device_work(kw, word):
    assert call(opts(**kw)) < 0
    assert word in _lib.lib().sf_last_error_string()


def test_the_limit_counts_every_row_of_the_call():
    # B * steps * V = 1024 * 1024 * 4096 = 2^32 with row_base 0
    assert call(opts(sample=1, inv_temperature=1.), B=1024, steps=1024) < 0
    assert b'2^32' in _lib.lib().sf_last_error_string()


def test_a_decoder_the_fused_step_refuses_is_an_error_with_an_option_on():
    small = desc(d=48, heads=3)   # d_model % 32 != 0
    assert _lib.lib().sf_slate_step_ok(C.byref(small)) == 0
    for o in (opts(sample=1, inv_temperature=1.), opts(soft_rows=16, conv0_t=16, conv0_width=64, soft_scale=10.)):
        assert call(o, m=small) < 0
        assert b'fused step' in _lib.lib().sf_last_error_string()
    # the errors of the plain entry point are those of the new one with no option
    for o in (None, opts()):
        one = C.c_void_p(16)
        assert _lib.lib().sf_slate_generate_tok_opts_f32(C.byref(desc()), None, 1, 1, one, None, 0, one, 1 << 40, None, None,
                                                         None if o is None else C.byref(o)) < 0
        assert b'null pointer' in _lib.lib().sf_last_error_string()


def test_python_refusals():
    from slotformer_amd import steve_render
    from slotformer_amd.base_slots.models.dVAE import dVAE
    from slotformer_amd.base_slots.models.steve_transformer import STEVETransformerDecoder
    dec = STEVETransformerDecoder(64, 64, 4, 15, 4, 1).eval()
    assert dec.step_ok()
    refused = STEVETransformerDecoder(32, 48, 3, 15, 3, 1).eval()
    assert not refused.step_ok()
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            refused.generate(torch.zeros(1, 3, 48), 4, sample=True, seed=3)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            dec.generate_tokens(torch.zeros(2, 4, 64), 4, sample=True, sample_seed=1)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            dVAE(64).eval().detokenize_rows(torch.zeros(1, 4, 4, 64))
    with pytest.raises(ValueError, match='gumbel'):
        steve_render.render_slots(dec, dVAE(64).eval(), torch.zeros(1, 4, 64), soft=True, fused=True, gumbel=torch.zeros(1, 64, 4, 4))


@pytest.mark.parametrize('start', [0, 1, 77, 4096 * 5, 2**32 - 50])
def test_gumbel_noise_at_an_offset_is_a_slice_of_the_sequence(start):
    seed = 0x1234567890abcdef
    assert torch.equal(train.gumbel_noise(seed, 50, start=start), train.gumbel_noise(seed, 50, start))
    if start <= 4096 * 5:
        whole = train.gumbel_noise(seed, start + 50)
        assert torch.equal(train.gumbel_noise(seed, 50, start=start), whole[start:])
    else:   # too long to build from zero: overlapping windows agree
        assert torch.equal(train.gumbel_noise(seed, 50, start=start)[10:], train.gumbel_noise(seed, 40, start=start + 10))
    assert torch.equal(train.gumbel_noise(seed, 9), train.gumbel_noise(seed, 9, start=0))


@pytest.mark.parametrize('seed', sc.CHI2_SEEDS)
def test_gumbel_max_on_the_twin_draws_from_the_softmax(seed):
    p = torch.softmax(torch.linspace(-1, 1, 32, dtype=torch.float64), 0)
    draws = sc.gumbel_max_draws(torch.log(p).expand(sc.DRAWS, 32), seed)
    chi2 = sc.chi_square(torch.bincount(draws, minlength=32), p)
    print('seed', seed, 'chi-square', chi2, 'smallest expected count', float(p.min()) * sc.DRAWS)
    assert chi2 < sc.CHI2_31_999


@pytest.mark.parametrize('name', ['v40', 'v200'])
@pytest.mark.parametrize('seed', sc.SAMPLE_SEEDS)
@pytest.mark.parametrize('temperature', sc.TEMPERATURES)
def test_the_float64_sampled_run_has_no_near_tie(name, seed, temperature):
    """the rule of test_tokens_and_logits_against_float64: smallest top-2 margin above 1e-4 of max|score|, at every position of every frame"""
    idx, logits, margin = sc.sampled_run64(name, seed, temperature)
    print(name, 'seed', seed, 'T', temperature, 'smallest top-2 score margin / max|score|', margin)
    assert tuple(idx.shape) == (sc.FRAMES, sc.STEPS) and margin > 1e-4
    greedy = logits.argmax(-1)
    assert not torch.equal(greedy, idx)      # the noise does change the choice: the GPU test cannot pass on the greedy path
