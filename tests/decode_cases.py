"""Decoder shapes shared by tests/test_decode_cases.py (CPU) and tests/test_decode_gpu.py: each is the smallest StoSAVi decoder that still takes
one branch of sf_savi_decode_seg_f32, with the mask-logit row of the head scaled up so that the segmentation rule has something to decide
(with plain seeded weights every mask value stays below the threshold and every frame is one label), and the float64 reference of each."""
import functools

import torch

import golden_util as gu
import oracle

SD_SEED, SLOT_SEED, MASK_GAIN = 7, 9, 64.
FG_THRE = 0.5
MARGIN = 1e-4      # a pixel nearer than this to a decision of the segmentation rule is not compared against the float64 segmentation

# name -> (res, N, D, dec_channels, dec_res, ks, F)
CASES = {
    # C5_SAVI's decoder: fold at 16, W = 32 and W = 64 plain fragment layers, generic stride-1 layer at 128, separate head GEMM
    'phyre': (128, 8, 128, (128, 64, 64, 64, 64), 16, 5, 2),
    # a stride-1 layer that is not the last (flipped generic convolution), then the fused rows4 + head last layer
    'two_s1': (64, 6, 128, (128, 64, 64, 64, 64), 16, 5, 2),
    # fold with C1 = 32; no fragment kernel applies afterwards
    'c32': (64, 7, 128, (128, 32, 32, 32, 32), 8, 5, 2),
    # fold at dec_res 2 (the border classes collide); HW = 256: one workgroup per frame
    'tiny2': (16, 3, 32, (32, 16, 16, 16, 16), 2, 5, 5),
    # fold refused: slot_broadcast; N > 8; HW = 16 (HW % 256 != 0, F * HW < 256)
    'res1': (4, 11, 16, (16, 8, 8), 1, 5, 3),
    # dec_ks 3; N = 16 (the limit)
    'ks3': (16, 16, 32, (32, 16, 16), 4, 3, 2),
}
NAMES = list(CASES)


def case_cfg(name):
    res, N, D, ch, r, ks, _ = CASES[name]
    cfg = gu.savi_cfg(res, N, slot_size=D, dec_res=(r, r))
    cfg['dec_dict'] = dict(dec_channels=tuple(ch), dec_resolution=(r, r), dec_ks=ks, dec_norm='')
    return cfg


def case_slots(name, F=None, seed=SLOT_SEED):
    _, N, D, _, _, _, F0 = CASES[name]
    return gu.seeded_normal((F0 if F is None else F, N, D), seed)


def build_case(name, gain=MASK_GAIN, seed=SD_SEED):
    """(module on the CPU in eval mode, float64 state dict, cfg): seeded weights, row 3 (the mask logit) of the 1x1 head times `gain`"""
    from slotformer_amd.base_slots import build_model
    cfg = case_cfg(name)
    m = build_model(gu.ParamsView(cfg)).eval()
    own = m.state_dict()
    sd = gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in own.items()], seed, keep=own)
    head = f'decoder.{len(CASES[name][3]) - 1}.weight'
    assert tuple(sd[head].shape[:2]) == (4, CASES[name][3][-1]), head
    sd[head][3] *= gain
    m.load_state_dict(sd)
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    return m, sd64, cfg


def segmentation_facts(masks):
    """masks [F,N,1,H,W] (float64 reference) -> dict of [F,HW] tensors: best mask value, `excluded` (the pixels whose segmentation the
    float32 decoder may legitimately decide the other way), and the reference segmentation [F,H,W]."""
    F_, N, _, H, W = masks.shape
    m = masks.reshape(F_, N, H * W)
    top2 = m.topk(2, dim=1)[0]
    best = top2[:, 0]
    below = best < FG_THRE
    peaks = m.max(-1)[0].sort(-1)[0]
    ambiguous = (peaks[:, 1] - peaks[:, 0]) <= MARGIN                   # frames whose background slot is not settled
    tie = (top2[:, 0] - top2[:, 1]) <= MARGIN
    edge = (best - FG_THRE).abs() <= MARGIN
    excluded = tie | edge | (below & ambiguous[:, None])
    return dict(best=best, below=below, tie=tie, edge=edge, ambiguous=ambiguous, excluded=excluded,
                seg=oracle.postproc_mask(masks.unsqueeze(0), FG_THRE)[0])


@functools.lru_cache(maxsize=None)
def reference(name, F=None, frames=None):
    """float64 decode of the case's slots (of F frames instead of the case's own; of the frames of the tuple `frames` only):
    dict(recon, recons, masks, logits) + segmentation_facts.  Computed once; do not write into it."""
    _, sd64, cfg = build_case(name)
    slots = case_slots(name, F).double()
    if frames is not None:
        slots = slots[list(frames)]
    with torch.no_grad():
        recon, recons, masks, logits = oracle.savi_decode(slots, sd64, cfg, return_logits=True)
    out = dict(recon=recon, recons=recons, masks=masks, logits=logits)
    out.update(segmentation_facts(masks))
    return out
