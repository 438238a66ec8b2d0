"""The FFN block of the token-stationary layer launch on v_mfma_f32_16x16x32_bf16 (csrc/layer_tok.hip, the lt16_* helpers of csrc/layer_tok_common.h):
the kernel against the float64 restatement of the layer at the smallest shapes where the 16-token tiles, the layout swaps at the two borders of the block
and the feature permutation of its vectors can go wrong; the packed blob decoded on the host with the element map the headers document; the C2 rollout
against the reference's fixture and against the default forms."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from test_layer_tok_gpu import _layer64, _rollouter

pytestmark = pytest.mark.gpu

# (videos, tokens per video): three videos with two padding rows; one video with idle waves; several videos inside ONE 16-token tile; a video boundary
# that is not on a 16-row boundary; one video per workgroup; the last key block; videos exactly on tile boundaries
SHAPES = [(3, 42), (1, 42), (2, 7), (7, 40), (4, 50), (3, 96), (35, 16)]


@functools.lru_cache(maxsize=None)
def _model(dev):
    """the rollouter (weights from the initialiser, every vector drawn per element: _rollouter moves biases and LayerNorm parameters off 0 / 1) and its plan"""
    from slotformer_amd import engine
    r = _rollouter(dev)
    return r, engine.rollouter_plan(r)


@functools.lru_cache(maxsize=None)
def _case(dev, B, L):
    """input and the float64 outputs behind one and three layers: computed once, never written to"""
    r, _ = _model(dev)
    x = gu.seeded_normal((B, L, 256), 100 * B + L).to(dev)
    refs, ref = {}, x
    with torch.no_grad():
        for k in range(3):
            ref = _layer64(r.transformer_encoder.layers[k], ref)
            refs[k + 1] = ref
    return x, refs


def _run(plan, nl, x):
    from slotformer_amd import _lib
    B, L, _ = x.shape
    y = torch.full((B, L, 256), float('nan'), device=x.device)
    _lib.check(_lib.lib().sf_layer_tok_block_f32(plan.struct.layers, nl, x.data_ptr(), y.data_ptr(), B, L, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('B,L', SHAPES)
@pytest.mark.parametrize('nl', [1, 3])
@torch.no_grad()
def test_layer_tok_shape_vs_float64(dev, B, L, nl):
    _, plan = _model(dev)
    x, refs = _case(dev, B, L)
    ref = refs[nl]
    y = _run(plan, nl, x)
    err = ((y.double() - ref).abs().max() / ref.abs().max()).item()
    print(f'B {B} L {L} layers {nl}: rel err vs float64 {err:.2e}')
    assert err < 1e-5
    # a video's bits do not depend on the other videos of the call
    if B >= 2:
        x2 = gu.seeded_normal((B, L, 256), 7).to(dev)
        keep = B // 2
        x2[keep] = x[keep]
        assert torch.equal(_run(plan, nl, x2)[keep], y[keep])
    # two calls give equal bits
    assert torch.equal(_run(plan, nl, x), y)


def _feat16(g):
    return 8 * (g & 1) + 4 * (g >> 1)


def _element_map():
    """(matrix, row, column) of every bf16 element of a plane, [96 stages][16 fragments of the plane][64 lanes][8], as layer_tok_common.h documents it:
    matrix 0 in_proj_w [768][256], 1 out_proj_w [256][256], 2 lin1_w [1024][256], 3 lin2_w [256][1024]; the plane of fragment f is f & 1"""
    NB, NFF = 8, 64
    lane, j = np.meshgrid(np.arange(64), np.arange(8), indexing='ij')
    mat = np.zeros((96, 16, 64, 8), np.int64)
    row = np.zeros_like(mat)
    col = np.zeros_like(mat)
    # attention stages, 32x32x16 fragments: lane (i, h), element j of k-step s over columns c0 ..: W[r0 + i][c0 + 8 (2 s + (j >> 2)) + 4 h + (j & 3)]
    i32, h32 = lane & 31, lane >> 5
    for st in range(4 * NB):
        if st < 3:
            hd, kind = 0, st
        elif st == 4 * NB - 1:
            hd, kind = NB - 1, 3
        else:
            kind = (st - 3) & 3
            hd = 1 + ((st - 3) >> 2) - (1 if kind == 3 else 0)
        for fp in range(16):
            if kind < 3:    # row stage: fragment pair = virtual k-step (input block ib, s)
                ib, s = fp >> 1, fp & 1
                mat[st, fp], row[st, fp], col[st, fp] = 0, kind * 256 + 32 * hd + i32, 32 * ib + 8 * (2 * s + (j >> 2)) + 4 * h32 + (j & 3)
            else:           # column stage: fragment pair = (output block ob, s)
                ob, s = fp >> 1, fp & 1
                mat[st, fp], row[st, fp], col[st, fp] = 1, 32 * ob + i32, 32 * hd + 8 * (2 * s + (j >> 2)) + 4 * h32 + (j & 3)
    # FFN stages, 16x16x32 fragments: lane (i = lane & 15, g = lane >> 4)
    i16, g16 = lane & 15, lane >> 4
    for ff in range(NFF):
        st = 4 * NB + ff
        if ff == 0:
            slc, hb = False, 0
        elif ff == NFF - 1:
            slc, hb = True, 31
        elif ff & 1:
            slc, hb = False, (ff + 1) >> 1
        else:
            slc, hb = True, (ff >> 1) - 1
        for fp in range(16):
            if not slc:     # lin1 rows of hidden block hb: fragment pair = (k-step ks, row half r)
                ks, r = fp >> 1, fp & 1
                mat[st, fp], row[st, fp], col[st, fp] = 2, 32 * hb + 16 * r + i16, 32 * ks + 16 * (j >> 2) + _feat16(g16) + (j & 3)
            else:           # lin2 columns of hidden block hb: fragment pair = 16-row output block ob
                mat[st, fp], row[st, fp], col[st, fp] = 3, 16 * fp + _feat16(i16 >> 2) + (i16 & 3), 32 * hb + 16 * (j >> 2) + 4 * g16 + (j & 3)
    return mat, row, col


@torch.no_grad()
def test_layer_tok_blob_decodes_to_the_weights(dev):
    """Every weight of a random layer, hi = bf16(w) and lo = bf16(w - hi), exactly once per plane and where the documented element map puts it"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(16)
    shapes = {'norm1_g': (256, ), 'norm1_b': (256, ), 'in_proj_w': (768, 256), 'in_proj_b': (768, ), 'out_proj_w': (256, 256), 'out_proj_b': (256, ),
              'norm2_g': (256, ), 'norm2_b': (256, ), 'lin1_w': (1024, 256), 'lin1_b': (1024, ), 'lin2_w': (256, 1024), 'lin2_b': (256, )}
    t = {k: torch.randn(*s, generator=g).to(dev) for k, s in shapes.items()}
    w = _lib.sf_tfm_layer()
    for k, v in t.items():
        setattr(w, k, v.data_ptr())
    nb = lib.sf_layer_tok_packed_bytes()
    assert nb == 96 * 32768 + 3328 * 4
    blob = torch.zeros(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.sf_pack_layer_tok_weights(C.byref(w), blob.data_ptr(), 256, 8, 1024, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = blob.cpu().numpy()
    frag = host[:96 * 32768].view(np.uint16).reshape(96, 16, 2, 64, 8)    # [stage][fragment pair][plane][lane][element]
    mats = [t[k].cpu() for k in ('in_proj_w', 'out_proj_w', 'lin1_w', 'lin2_w')]
    hi = [m.to(torch.bfloat16) for m in mats]
    lo = [(m - h.float()).to(torch.bfloat16) for m, h in zip(mats, hi)]
    bits = lambda b: b.view(torch.int16).numpy().view(np.uint16)  # noqa: E731
    mat, row, col = _element_map()
    off = np.cumsum([0] + [m.numel() for m in mats])
    flat = off[mat] + row * np.array([m.shape[1] for m in mats])[mat] + col
    assert np.array_equal(np.bincount(flat.ravel(), minlength=off[-1]), np.ones(off[-1], np.int64))    # every weight once per plane
    for pl, planes in enumerate((hi, lo)):
        want = np.concatenate([bits(p).ravel() for p in planes])[flat]
        assert np.array_equal(frag[:, :, pl], want), ('hi', 'lo')[pl]
    vec = host[96 * 32768:].view(np.float32)
    order = ('norm1_g', 'norm1_b', 'in_proj_b', 'out_proj_b', 'norm2_g', 'norm2_b', 'lin1_b', 'lin2_b')
    assert np.array_equal(vec, np.concatenate([t[k].cpu().numpy() for k in order]))


@torch.no_grad()
def test_rollout_c2_with_layer_tok(dev):
    """roll_c2 (B = 2, 50 steps) with the token-stationary layers against the reference's fixture, and against the default forms"""
    from test_engine_gpu import build
    from slotformer_amd import engine
    cfg, B, pred_len, seed = gu.C2_ROLL, 2, 50, 202
    g = gu.load_golden('roll_c2')
    m, _ = build(cfg, g, seed, dev, vp=True)
    rd = cfg['rollout_dict']
    hist, N, Cs = rd['history_len'], rd['num_slots'], rd['slot_size']
    T_in = engine.burn_in_of(m.rollouter)
    slots = gu.seeded_normal((B, hist + pred_len, N, Cs), seed + 1).to(dev)
    buf = torch.zeros(B, T_in + pred_len, N, Cs, device=dev)
    buf[:, :T_in] = slots[:, :T_in]
    engine.rollout(m.rollouter, buf, T_in, pred_len, opts={'layer_tok': True})
    ref = torch.as_tensor(g['pred_slots']).to(dev)
    e = ((buf[:, T_in:] - ref).abs().max() / ref.abs().max()).item()
    other = buf.clone()
    other[:, T_in:] = 0
    engine.rollout(m.rollouter, other, T_in, pred_len, opts={'layer_tok': False})
    d = ((buf - other).abs().max() / ref.abs().max()).item()
    print(f'roll_c2: token-stationary layers vs the fixture {e:.2e}, vs the default forms {d:.2e}')
    assert e < 5e-5
    assert 0 < d < 2e-5
