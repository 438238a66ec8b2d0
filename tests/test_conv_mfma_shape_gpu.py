"""The 5x5 / 64 -> 64 convolutions on v_mfma_f32_16x16x32_bf16 (sf_conv_tile16, csrc/split_bf16.h): the weights-stationary kernel (conv_ws.hip),
the 4-row-tile kernel (conv_rows4.hip) and the 2-row halo kernel (conv_halo.hip) against float64 at the smallest shapes that reach every branch
of the row walk, bit for bit against each other, the fragment packer's layout, and non-finite inputs.

The bound is the one test_conv5x5_ws (test_kernels_gpu.py) holds the kernels to on the same input distribution: max |err| <= 1e-4 + 1e-4 max |ref|
(split-bf16 keeps ~16 mantissa bits per operand: 2^-17 relative per product, 1600 products of size ~0.03 per output).  The 4-row-tile kernel takes
H % 4 == 0 and the halo kernel H % 2 == 0: a kernel meets the shapes it takes, and (1, 4), (2, 8) are there so that all three meet."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (1, 5), (1, 6), (2, 3), (3, 7), (1, 4), (2, 8)]
# (bias, relu, per-position table)
OPTIONS = [(True, True, True), (False, False, False), (True, True, False), (False, False, True)]
RTOL = ATOL = 1e-4


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(F_, H):
    """Inputs of a shape and the float64 convolution without bias / ReLU / table (shared by every option: those are added in float64 below)."""
    x, w, b, add = rnd(F_, H, 64, 64, seed=1), rnd(64, 64, 5, 5, seed=2, scale=0.03), rnd(64, seed=3, scale=0.1), rnd(H * 64, 64, seed=4)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, padding=2).permute(0, 2, 3, 1).contiguous()
    return x, w, b, add, ref


def reference(F_, H, bias, relu, table):
    x, w, b, add, ref = case(F_, H)
    if bias:
        ref = ref + b.double()
    if relu:
        ref = F.relu(ref)
    if table:
        ref = ref + add.double().view(1, H, 64, 64)
    return ref


def over_bound(out, ref):
    """max |err| as a fraction of the bound."""
    err = (out.detach().cpu().double() - ref).abs().max().item()
    return err / (ATOL + RTOL * ref.abs().max().item())


@functools.lru_cache(maxsize=None)
def weights(dev):
    from slotformer_amd import ops
    w = case(1, 1)[1]
    wp = ops.pack_conv_weight(w.to(dev))
    return wp, ops.pack_conv_frag(wp)


def forms(dev, F_, H, bias, relu, table):
    """name -> output of every form that takes the shape (the weights-stationary kernel for each split of the rows)."""
    from slotformer_amd import ops
    x, w, b, add, _ = case(F_, H)
    wp, wf = weights(dev)
    xd, bd, ad = x.to(dev), (b.to(dev) if bias else None), (add.to(dev) if table else None)
    outs = {}
    for nwg in sorted({1, 2, 3, F_ * H}):
        if nwg <= F_ * H:
            outs[f'ws/{nwg}'] = ops.conv5x5_ws(xd, wf, bd, relu=relu, add=ad, n_workgroups=nwg)
    if H % 4 == 0:
        outs['rows4'] = ops.conv5x5_frag(xd, wf, bd, relu=relu, add=ad)
    if H % 2 == 0:
        outs['halo'] = ops.conv2d_nhwc(xd, wp, bd, relu=relu, add=ad)
    return outs


@pytest.mark.parametrize('F_,H', SHAPES)
@pytest.mark.parametrize('bias,relu,table', OPTIONS)
def test_product_against_float64(dev, F_, H, bias, relu, table):
    """Every form against float64 at the bound of test_conv5x5_ws, and all forms bit for bit the same."""
    ref = reference(F_, H, bias, relu, table)
    outs = forms(dev, F_, H, bias, relu, table)
    worst = {k: over_bound(v, ref) for k, v in outs.items()}
    print(f'F={F_} H={H} bias={bias} relu={relu} table={table}: max err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    first = outs['ws/1']
    for k, v in outs.items():
        assert torch.equal(v, first), (k, (v - first).abs().max().item())


def test_fragment_packer_layout(dev):
    """sf_pack_conv_frag_weights: uint4 index ((((tap * 2 + kh) * 2 + cb) * 2 + a) * 2 + plane) * 64 + lane holds
    w[cb * 32 + 16 a + (lane & 15)][tap][kh * 32 + 8 (lane >> 4) + j], j = 0 .. 7, plane 0 = bf16(w), plane 1 = bf16(w - plane 0)."""
    from slotformer_amd import ops
    w = rnd(64, 64, 5, 5, seed=11, scale=0.3)
    wp = ops.pack_conv_weight(w.to(dev))                      # [cout][ky][kx][cin]
    frag = ops.pack_conv_frag(wp)[:409600].cpu()
    got = frag.view(torch.bfloat16).view(25, 2, 2, 2, 2, 64, 8)   # tap, kh, cb, a, plane, lane, j
    lane = torch.arange(64)
    planes = torch.empty(2, 64, 25, 64, dtype=torch.bfloat16)
    for kh in range(2):
        for cb in range(2):
            for a in range(2):
                cout = cb * 32 + 16 * a + (lane & 15)                                   # [lane]
                cin = kh * 32 + 8 * (lane >> 4)[:, None] + torch.arange(8)[None]        # [lane][j]
                for pl in range(2):
                    for tap in range(25):
                        planes[pl, cout[:, None].expand(64, 8), tap, cin] = got[tap, kh, cb, a, pl]
    wf32 = wp.cpu().view(64, 25, 64)
    hi = wf32.to(torch.bfloat16)
    lo = (wf32 - hi.float()).to(torch.bfloat16)
    assert torch.equal(planes[0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(planes[1].view(torch.int16), lo.view(torch.int16))


@pytest.mark.parametrize('F_,H', [(3, 7), (2, 8)])
def test_non_finite_inputs_stay_where_they_are(dev, F_, H):
    """One NaN and one inf in a frame come out non-finite at exactly the outputs whose 5x5 window holds them (no ReLU: its max would map a NaN to
    0 by definition); the rows of zeros between frames are selects and must not launder or spread them."""
    from slotformer_amd import ops
    x, w, b, add, _ = case(F_, H)
    wp, wf = weights(dev)
    x = x.clone()
    spots = [(F_ - 1, 0, 1, 5, float('nan')), (0, H - 1, 62, 40, float('inf'))]
    expect = torch.zeros(F_, H, 64, 64, dtype=torch.bool)
    for f, y, px, c, v in spots:
        x[f, y, px, c] = v
        expect[f, max(y - 2, 0):y + 3, max(px - 2, 0):px + 3, :] = True
    xd, bd = x.to(dev), b.to(dev)
    outs = {f'ws/{n}': ops.conv5x5_ws(xd, wf, bd, relu=False, n_workgroups=n) for n in (1, 2, 3, F_ * H)}
    if H % 4 == 0:
        outs['rows4'] = ops.conv5x5_frag(xd, wf, bd, relu=False)
        outs['halo'] = ops.conv2d_nhwc(xd, wp, bd, relu=False)
    for k, v in outs.items():
        bad = ~torch.isfinite(v.cpu())
        assert torch.equal(bad, expect), (k, int(bad.sum()), int(expect.sum()))
