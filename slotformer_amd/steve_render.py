"""STEVE slots -> frames on the device (the rendering of steve_slotformer.py:86-103 and base_slots/method.py:353-378).

`render_slots` generates the dVAE token grid of every frame greedily with the slot-conditioned Transformer decoder
(`STEVETransformerDecoder.generate_tokens`: one launch per token where the fused step applies, tokens and logits left on the
device) and detokenises it: the hard image from the token ids by a row gather (`dVAE.detokenize_ids`), the soft image from the
Gumbel-softmax relaxation of the logits at tau = 0.1.  Nothing travels through host memory.  Inference only.

With `fused=True` the relaxation and the first dVAE decoder block run inside the token step's vocabulary sweep: the step hands back
64 numbers per token (`generate_tokens(soft_table=...)` -> `dVAE.detokenize_rows`) and no [F, h*w, V] buffer exists.  With
`sample=True` the tokens are drawn from softmax(logits / temperature) inside the step instead of taken greedily."""
import torch

from . import ops

GUMBEL_TAU = 0.1   # steve_slotformer.py:98, base_slots/method.py:368


def _fresh_seed():
    return int(torch.randint(0, 2**62, (1, )).item())


def render_slots(decoder, dvae, slots, soft=False, gumbel=None, seed=None, frames_per_wg=0, fused=False, first_frame=0, sample=False,
                 temperature=1.0, sample_seed=None):
    """slots [F,N,D] float32 on the device -> {'tokens': int64 [F,h,w], 'hard': [F,3,H,W]} and, with soft=True, 'soft': [F,3,H,W];
    all on the device.  `decoder` is a STEVETransformerDecoder over h * w = decoder.max_len + 1 tokens (a square grid), `dvae` the
    tokenizer it was trained with.  hard detokenises the argmax tokens; soft detokenises softmax((logits + g) / 0.1), g being the
    caller's `gumbel` [F,V,h,w] or Gumbel(0, 1) noise generated inside the softmax kernel from `seed` (default: a fresh one).
    The logits [F,h*w,V] are only materialised with soft=True.  A frame's result does not depend on the other frames of the call (as long as the
    library picks the same generation form for both batch sizes): rendering in chunks gives the bits of one call.

    fused=True (with soft=True): the soft image comes from the soft rows of the fused token step, the same noise of `seed` added inside its
    vocabulary sweep, and neither the logits nor the relaxation [F,h*w,V] is allocated; `gumbel=` cannot be combined with it (ValueError), and
    where the fused step refuses the decoder the route above runs.  sample=True: the tokens (and so the hard image) are drawn from
    softmax(logits / temperature) inside the fused step with the noise of `sample_seed` (default: a fresh one).  `first_frame`: the index of
    slots[0] in the sequence the caller renders, so that the noise of a sequence rendered in several calls is the noise of one call (it
    offsets the rows of the in-step noise; the softmax kernel of the unfused route always counts from the start of its call)."""
    if fused and gumbel is not None:
        raise ValueError('render_slots: fused=True draws its noise inside the token step; it cannot take gumbel=')
    if decoder.training or dvae.training or torch.is_grad_enabled():
        raise RuntimeError('slotformer_amd STEVETransformerDecoder is inference-only: .eval() + torch.no_grad()')
    if not (torch.is_tensor(slots) and slots.is_cuda and slots.dtype == torch.float32):
        raise RuntimeError('render_slots needs float32 slots on a HIP device; there is no CPU fallback')
    assert slots.dim() == 3, 'slots are [F, N, D]'
    P = decoder.max_len + 1
    h = int(round(P**0.5))
    assert h * h == P, f'the decoder generates {P} tokens: not a square grid'
    F_ = slots.shape[0]
    fused = bool(fused and soft and decoder.step_ok())
    kw = {}
    if sample:
        kw.update(sample=True, temperature=temperature, sample_seed=_fresh_seed() if sample_seed is None else sample_seed)
    if fused or sample:
        kw['row_base'] = int(first_frame) * P
    if fused:
        seed = _fresh_seed() if seed is None else seed
        tokens, logits, rows = decoder.generate_tokens(slots, P, frames_per_wg=frames_per_wg, soft_table=dvae.conv0_table(),
                                                       soft_scale=1.0 / GUMBEL_TAU, soft_seed=seed, **kw)
    else:
        tokens, logits = decoder.generate_tokens(slots, P, return_logits=bool(soft), frames_per_wg=frames_per_wg, **kw)
    tokens = tokens.view(F_, h, h)
    # frame by frame: the GEMMs of the dVAE pick their tiles by the row count, so a frame's bits would depend on the size of the call;
    # next to a thousand token steps per frame the extra launches cost nothing
    out = {'tokens': tokens, 'hard': torch.cat([dvae.detokenize_ids(tokens[i:i + 1]) for i in range(F_)])}
    if fused:
        rows = rows.view(F_, h, h, rows.shape[-1])
        out['soft'] = torch.cat([dvae.detokenize_rows(rows[i:i + 1]) for i in range(F_)])
    elif soft:
        if gumbel is not None:
            assert tuple(gumbel.shape) == (F_, decoder.vocab_size, h, h), 'gumbel is [F, V, h, w]'
            noise = gumbel.to(logits.device).float().flatten(2, 3).transpose(1, 2).contiguous()
            z = ops.softmax_rows(logits, noise, 1.0 / GUMBEL_TAU)
        else:
            z = ops.gumbel_softmax_rows(logits, _fresh_seed() if seed is None else seed, 1.0 / GUMBEL_TAU)
        z = z.view(F_, h, h, decoder.vocab_size)
        out['soft'] = torch.cat([dvae.detokenize_nhwc(z[i:i + 1]) for i in range(F_)])
    return out
