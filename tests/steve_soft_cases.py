"""Shared by test_steve_soft_render.py (CPU) and test_steve_soft_render_gpu.py: the decoders, slots and float64 restatements of what the fused
token step computes in its head epilogue -- the soft rows (Gumbel-softmax relaxation times the first dVAE decoder block) and the Gumbel-max draw.
Everything here runs on the CPU in float64 on top of `oracle.steve_decoder_forward` and the host twin of the kernel's noise,
`train.gumbel_noise`; results are computed once per process and never modified."""
import functools

import torch

import golden_util as gu
import oracle
from slotformer_amd import train

FRAMES, STEPS = 5, 16     # 5 frames: a ragged last workgroup at 2 and 4 frames per workgroup; 16 steps: a 4 x 4 token grid
SOFT_SCALE = 10.0         # 1 / tau, tau = 0.1 (steve_slotformer.py:98)
CHI2_31_999 = 61.10       # 99.9 % quantile of chi-square at 31 degrees of freedom
DRAWS = 4096

CASES = {
    # name: ((V, d, heads, max_len, slots, blocks), weights seed, slots seed)
    'v40': ((40, 32, 2, 15, 2, 1), 911, 1911),      # most of the 128 weight-row groups see no word
    'v200': ((200, 64, 4, 15, 4, 2), 912, 1912),    # some groups take one word, some two; V is no multiple of 128
    'v32': ((32, 32, 2, 0, 2, 1), 913, 1913),       # one step: the draw statistics
}
# Seeds picked on the CPU (see test_steve_soft_render.py): the float64 sampled runs of v40 and v200 have no near tie at any position for these, and
# Gumbel-max on the twin's noise passes the chi-square bound for each of CHI2_SEEDS.
SAMPLE_SEEDS = (23, 24)
TEMPERATURES = (1.0, 0.5)
CHI2_SEEDS = (31, 32, 33)


def rel_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max()).item()


def make_decoder(shape, seed, prefix='trans_decoder.'):
    """(module on the CPU in eval mode, state dict under the oracle's names)"""
    from slotformer_amd.base_slots.models.steve_transformer import STEVETransformerDecoder
    dec = STEVETransformerDecoder(*shape)
    own = {prefix + k: v for k, v in dec.state_dict().items()}
    sd = gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in own.items()], seed, keep=own)
    dec.load_state_dict({k[len(prefix):]: v for k, v in sd.items()}, strict=True)
    return dec.eval(), sd


def make_dvae(V, seed):
    """(dVAE module on the CPU in eval mode, state dict under 'dvae.')"""
    from slotformer_amd.base_slots.models.dVAE import dVAE
    m = dVAE(V)
    own = {'dvae.' + k: v for k, v in m.state_dict().items()}
    sd = gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in own.items()], seed, keep=own)
    m.load_state_dict({k[len('dvae.'):]: v for k, v in sd.items()}, strict=True)
    return m.eval(), sd


def double_sd(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    shape, wseed, sseed = CASES[name]
    dec, sd = make_decoder(shape, wseed)
    slots = gu.seeded_normal((FRAMES, shape[4], shape[1]), sseed)
    table = gu.seeded_normal((shape[0], 64), wseed + 50) * 0.3     # a stand-in for the transposed first decoder block weight
    return dict(dec=dec, sd=sd, sd64=double_sd(sd), slots=slots, shape=shape, table=table)


def noise(seed, B, steps, V, row_base=0):
    """the noise the step adds to logits [B, steps, V]: element (row_base + b * steps + t) * V + v of the stream, float64"""
    return train.gumbel_noise(seed, B * steps * V, start=row_base * V).view(B, steps, V).double()


def soft_rows64(logits, table, seed, scale=SOFT_SCALE, row_base=0):
    """y[b, t, :] = softmax((l + G) * scale) @ table in float64, l being the logits handed in (the kernel's own)"""
    l = logits.detach().cpu().double()
    B, steps, V = l.shape
    z = torch.softmax((l + noise(seed, B, steps, V, row_base)) * scale, -1)
    return z @ table.double()


@functools.lru_cache(maxsize=None)
def sampled_run64(name, seed, temperature, steps=STEPS, row_base=0):
    """The float64 sampled generation (prefix re-run): token[b, t] = argmax_v(l_v / T + G(seed, r V + v)), fed back.  Returns tokens [B, steps],
    logits [B, steps, V] and the smallest top-2 margin of the score over max|score|."""
    c = case(name)
    shape = c['shape']
    B, V = FRAMES, shape[0]
    g = noise(seed, B, steps, V, row_base)
    idx = torch.zeros(B, 0, dtype=torch.long)
    logits, scores = [], []
    with torch.no_grad():
        for t in range(steps):
            lg = oracle.steve_decoder_forward(c['slots'].double(), idx, c['sd64'], shape[2], shape[5])[:, -1]
            score = lg / temperature + g[:, t]
            scores.append(score)
            logits.append(lg)
            idx = torch.cat([idx, score.argmax(-1, keepdim=True)], 1)
    scores = torch.stack(scores, 1)
    top2 = scores.topk(2, -1).values
    margin = ((top2[..., 0] - top2[..., 1]).min() / scores.abs().max()).item()
    return idx, torch.stack(logits, 1), margin


def chi_square(counts, probs):
    """Pearson's statistic of observed counts against expected probabilities (float64)"""
    counts, probs = counts.double(), probs.double()
    e = probs * counts.sum()
    return float(((counts - e)**2 / e).sum())


def gumbel_max_draws(logits, seed, inv_temperature=1.0):
    """one Gumbel-max draw per row of logits [R, V] (float64) with the twin's noise of rows 0..R-1"""
    R, V = logits.shape
    return (logits.double() * inv_temperature + train.gumbel_noise(seed, R * V).view(R, V).double()).argmax(-1)
