"""Seeded weights, inputs and float64 restatements shared by tests/test_dvae_tokens.py (CPU) and tests/test_dvae_tokens_gpu.py: the vocabulary
head with the argmax inside (csrc/dvae_tokens.hip), the patch embedding, and the whole dVAE encoder.

The comparison rule is the project's own (tests/test_engine_gpu.py, test_steve_image_side_golden): a position is SAFE when the float64 gap between
its two best logits exceeds SAFE_REL x max|logit| of the case; device ids must equal the float64 ids on every safe position, and overall no more
positions may differ than there are unsafe ones.  A case may have at most MAX_UNSAFE of its positions unsafe -- asserted on the CPU of every case
the GPU tests use, so a badly chosen seed fails there and not silently on the GPU.

Every case is computed once per process and shared: treat what these functions return as read-only."""
import functools

import torch
import torch.nn.functional as F

SAFE_REL = 1e-4
MAX_UNSAFE = 0.02
PARITY = 1e-3

HEAD_ROWS = (1, 63, 64, 65, 257, 1000)   # a wave's tile is 64 rows, a workgroup's 64 or 256: one partly filled wave ... 15.6 waves
HEAD_VOCABS = (64, 512, 4096)
HEAD_LD = 80                             # the strided variant: rows of 64 features inside rows of 80 floats (16-byte aligned: 320 bytes)
PATCH_CASES = ((1, 8, 8), (3, 20, 36), (2, 64, 64), (2, 128, 128))   # (F, H, W): 4, 135, 512 and 2048 tokens (0.06, 2.1, 8 and 32 wave tiles)
MODEL_CASES = ((4096, 2, 128, 128), (4096, 3, 64, 64), (4096, 3, 20, 36), (64, 2, 64, 64))   # (V, F, H, W)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def judge(logits64):
    """logits64 [..., V] float64 -> (ids int64 [...], safe bool [...])"""
    top = torch.topk(logits64, 2, dim=-1)
    gap = top.values[..., 0] - top.values[..., 1]
    return top.indices[..., 0], gap > SAFE_REL * logits64.abs().max()


def check_ids(got, ids, safe):
    """the safe rule; returns (differing positions, unsafe positions) for the test to print"""
    got = got.cpu().long().reshape(ids.shape)
    diff = int((got != ids).sum())
    assert torch.equal(got[safe], ids[safe]), f'{int((got[safe] != ids[safe]).sum())} safe positions differ'
    assert diff <= int((~safe).sum())
    return diff, int((~safe).sum())


# ---- the head alone ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_case(V, R=max(HEAD_ROWS)):
    """dict(x [R,64] >= 0, w [V,64] ~ N(0,1)/8, b [V] ~ 0.1 N(0,1), ids [R], safe [R]); a case of fewer rows is the first rows of this one"""
    g = gen(4100 + V)
    x = torch.randn(R, 64, generator=g).abs()
    w = torch.randn(V, 64, generator=g) / 8
    b = 0.1 * torch.randn(V, generator=g)
    ids, safe = judge(x.double() @ w.double().t() + b.double())
    return dict(x=x, w=w, b=b, ids=ids, safe=safe)


def head_rows(V, R):
    """the first R rows of head_case(V), judged with max|logit| of those rows"""
    c = head_case(V)
    ids, safe = judge(c['x'][:R].double() @ c['w'].double().t() + c['b'].double())
    return dict(x=c['x'][:R], w=c['w'], b=c['b'], ids=ids, safe=safe)


@functools.lru_cache(maxsize=None)
def planted_case(V=4096):
    """R = V rows, row r built to make column c_r win (c a fixed permutation): x_r = 4 W[c_r] / |W[c_r]|, no bias"""
    g = gen(977)
    w = torch.randn(V, 64, generator=g) / 8
    c = torch.randperm(V, generator=g)
    x = 4 * w[c] / w[c].norm(dim=1, keepdim=True)
    ids, safe = judge(x.double() @ w.double().t())
    return dict(x=x, w=w, c=c, ids=ids, safe=safe)


def tie_groups(V):
    """list of (what, indices with IDENTICAL weight rows and bias).  A lane of the kernel holds words 8 g + 4 h + 0..3 of a block of 32 (h: the
    half-wave), so inside a block words 0-3, 8-11, ... sit in the lower half and 4-7, 12-15, ... in the upper one."""
    groups = [('index 0 and index V - 1', (0, V - 1)),
              ('the same block, one lane', (34, 42)),
              ('the same block, the two half-waves', (33, 37)),
              ('the same block, the later index in the lower half-wave', (44, 56)),
              ('different blocks', (7, 50)),
              ('three copies', (20, 27, 61))]
    if V >= 512:
        groups += [('blocks far apart', (100, 300)), ('three copies over three blocks, the later ones in the lower half-wave', (133, 264, 488)),
                   ('the last two blocks', (V - 40, V - 2))]
    return groups


@functools.lru_cache(maxsize=None)
def tie_case(V):
    """one row per group of tie_groups(V): x_r points along the group's weight row, so its members tie for the maximum; expected = the first"""
    g = gen(313 + V)
    w = torch.randn(V, 64, generator=g) / 8
    b = 0.1 * torch.randn(V, generator=g)
    groups = tie_groups(V)
    for _, idx in groups:
        w[list(idx[1:])] = w[idx[0]].clone()
        b[list(idx[1:])] = b[idx[0]].clone()
    first = torch.tensor([idx[0] for _, idx in groups])
    x = 4 * w[first] / w[first].norm(dim=1, keepdim=True)
    return dict(x=x, w=w, b=b, groups=groups, expected=first, logits=x.double() @ w.double().t() + b.double())


# ---- pack order ----------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 tensor (bf16-valued) -> its upper 16 bits as int32"""
    return (a.contiguous().view(torch.int32) >> 16) & 0xffff


def split(a):
    hi = a.bfloat16().float()
    return hi, (a - hi).bfloat16().float()


def packed_expected(w):
    """w [V,64] -> int32 [2, V/32, 4, 64, 8]: the bf16 bit patterns of (plane, block of 32 words, k-step, lane, element) by the formula of the header:
    lane l of block vb, k-step ks holds W[32 vb + (l & 31)][16 ks + 8 (l >> 5) + j]"""
    V = w.shape[0]
    hi, lo = split(w)
    out = torch.empty(2, V // 32, 4, 64, 8, dtype=torch.int32)
    lane = torch.arange(64)
    for ks in range(4):
        for j in range(8):
            col = 16 * ks + 8 * (lane >> 5) + j                                  # [64]
            row = 32 * torch.arange(V // 32)[:, None] + (lane & 31)[None, :]     # [V/32, 64]
            out[0, :, ks, :, j] = bf16_bits(hi)[row, col[None, :]]
            out[1, :, ks, :, j] = bf16_bits(lo)[row, col[None, :]]
    return out


# ---- patch embedding -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def patch_case(F_, H, W):
    """dict(img [F,3,H,W] ~ N(0,1), w [64,3,4,4] He-scaled, ref float64 [F,h,w,64], emu: the float32 emulation of split-bf16 on the same inputs)"""
    g = gen(55 + 1000 * H + W)
    img = torch.randn(F_, 3, H, W, generator=g)
    w = torch.randn(64, 3, 4, 4, generator=g) * (2. / 48) ** 0.5
    ref = F.conv2d(img.double(), w.double(), stride=4).permute(0, 2, 3, 1).contiguous()
    xh, xl = split(img)
    wh, wl = split(w)
    emu = (F.conv2d(xh, wl, stride=4) + F.conv2d(xl, wh, stride=4) + F.conv2d(xh, wh, stride=4)).permute(0, 2, 3, 1).double()
    return dict(img=img, w=w, ref=ref, emu=emu)


def rel(a, b):
    """max |a - b| / max |b|: the project's relative error of a tensor"""
    return ((a.double().cpu() - b.double()).abs().max() / b.double().abs().max()).item()


def patch_bound(c):
    """four times the distance of the emulation from float64 (the device sums in another order), never above the parity bar"""
    return min(4. * rel(c['emu'], c['ref']), PARITY)


# ---- the whole encoder ---------------------------------------------------------------------------------------------------------------------------
def seeded_dvae(V, seed=0):
    """a freshly constructed dVAE (its own initialisers) under a fixed seed, on the CPU, in eval mode"""
    from slotformer_amd.base_slots.models.dVAE import dVAE
    torch.manual_seed(9000 + 7 * V + seed)
    return dVAE(V).eval()


def encoder64(sd, imgs):
    """the dVAE encoder (dVAE.py:24-35) in float64 torch CPU operations: imgs [F,3,H,W] -> logits [F,h,w,V]"""
    x = imgs.double()
    for i in range(7):
        x = F.conv2d(x, sd[f'encoder.{i}.m.weight'].double(), stride=4 if i == 0 else 1)
        x = F.relu(F.group_norm(x, 1, sd[f'encoder.{i}.weight'].double(), sd[f'encoder.{i}.bias'].double(), 1e-5))
    return F.conv2d(x, sd['encoder.7.weight'].double(), sd['encoder.7.bias'].double()).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def model_case(V, F_, H, W, seed=0):
    """dict(sd, img [F,3,H,W] ~ N(0,1), ids [F,h,w], safe [F,h,w]) of a seeded model"""
    with torch.no_grad():
        sd = {k: v.clone() for k, v in seeded_dvae(V, seed).state_dict().items()}
        img = torch.randn(F_, 3, H, W, generator=gen(21 + V + 1000 * H + W + seed))
        ids, safe = judge(encoder64(sd, img))
    return dict(sd=sd, img=img, ids=ids, safe=safe)
