"""Decoder shapes shared by tests/test_decode_cases.py (CPU) and tests/test_decode_gpu.py: each is the smallest StoSAVi decoder that still takes
one branch of sf_savi_decode_seg_f32, with the mask-logit row of the head scaled up so that the segmentation rule has something to decide
(with plain seeded weights every mask value stays below the threshold and every frame is one label), and the float64 reference of each."""
import functools

import torch
import torch.nn.functional as F

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

# A seventh shape, for tests/test_savi_train_kernels_gpu.py alone (it is not in NAMES: the segmentation conditions of tests/test_decode_cases.py are not
# what it is built for).  The smallest decoder that still takes every launch of the training backward -- transposed convolutions 2 -> 4 -> 8 at stride 2
# and 8 -> 8 at stride 1: the generic weight-gradient kernel at s = 2 and s = 1, the strided and the masked GEMM adjoints, the head and broadcast
# kernels -- with weights under which no ReLU sits near its kink (train_case below), so that gradients compare element by element.
TRAIN_CASE = 'train8'
TRAIN_CASES = {TRAIN_CASE: (8, 2, 64, (64, 64, 64, 64), 2, 5, 2)}
TRAIN_SEED = 8
KINK_MARGIN = 1e-4      # of max |pre-activation of the layer|: the bound tests/test_conv_mfma_shape_gpu.py holds the convolutions to
MINORITY = 0.01         # at least this share of a layer's units is in the minority state of its channel
_ALL = dict(CASES, **TRAIN_CASES)


def case_cfg(name):
    res, N, D, ch, r, ks, _ = _ALL[name]
    cfg = gu.savi_cfg(res, N, slot_size=D, dec_res=(r, r))
    cfg['dec_dict'] = dict(dec_channels=tuple(ch), dec_resolution=(r, r), dec_ks=ks, dec_norm='')
    return cfg


def case_slots(name, F=None, seed=SLOT_SEED):
    _, N, D, _, _, _, F0 = _ALL[name]
    return gu.seeded_normal((F0 if F is None else F, N, D), seed)


def build_case(name, gain=MASK_GAIN, seed=SD_SEED):
    """(module on the CPU in eval mode, float64 state dict, cfg): seeded weights, row 3 (the mask logit) of the 1x1 head times `gain`"""
    from slotformer_amd.base_slots import build_model
    cfg = case_cfg(name)
    m = build_model(gu.ParamsView(cfg)).eval()
    own = m.state_dict()
    sd = gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in own.items()], seed, keep=own)
    head = f'decoder.{len(_ALL[name][3]) - 1}.weight'
    assert tuple(sd[head].shape[:2]) == (4, _ALL[name][3][-1]), head
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


def train_preactivations(slots, sd, cfg):
    """the pre-activation output of every transposed convolution of oracle.savi_decode (the same operations, in the dtype of slots / sd)"""
    dec = cfg['dec_dict']
    ch, ks, res, r = list(dec['dec_channels']), dec['dec_ks'], cfg['resolution'][0], dec['dec_resolution']
    Fr, N, D = slots.shape
    x = slots.reshape(Fr * N, D, 1, 1).repeat(1, 1, r[0], r[1])
    emb = F.linear(sd['decoder_pos_embedding.grid'], sd['decoder_pos_embedding.dense.weight'], sd['decoder_pos_embedding.dense.bias'])
    x = x + emb.permute(0, 3, 1, 2)
    size, stride, pre = r[0], 2, []
    for i in range(len(ch) - 1):
        if size == res:
            stride = 1
        z = F.conv_transpose2d(x, sd[f'decoder.{i}.0.weight'], sd.get(f'decoder.{i}.0.bias'), stride=stride, padding=ks // 2, output_padding=stride - 1)
        pre.append(z)
        x = F.relu(z)
        size *= stride
    return pre


@functools.lru_cache(maxsize=None)
def train_case():
    """(module on the CPU, float64 state dict, cfg, slots [F,N,D] float32) of TRAIN_CASE: seeded weights with the plain head (gain 1), the bias of every
    transposed convolution replaced by alternating +-2 standard deviations of the layer's bias-free response -- every channel is then mostly on or mostly off,
    a few percent of its units the other way, and no unit within KINK_MARGIN of zero (tests/test_savi_train_kernel_cases.py asserts both)."""
    m, sd64, cfg = build_case(TRAIN_CASE, gain=1., seed=TRAIN_SEED)
    slots = case_slots(TRAIN_CASE)
    L = len(_ALL[TRAIN_CASE][3]) - 1
    with torch.no_grad():
        for i in range(L):
            key = f'decoder.{i}.0.bias'
            sd64[key] = torch.zeros_like(sd64[key])
            z = train_preactivations(slots.double(), sd64, cfg)[i]
            sign = torch.tensor([2. if c % 2 == 0 else -2. for c in range(z.shape[1])], dtype=torch.float64)
            sd64[key] = (sign * z.std()).float().double()      # a float32 value: the module holds the same number
    m.load_state_dict({k: (v.float() if v.dtype.is_floating_point else v) for k, v in sd64.items()})
    return m, sd64, cfg, slots
