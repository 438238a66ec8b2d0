"""The references and tables of tests/steve_kernel_cases.py, held on the CPU to the conditions that tests/test_steve_kernels_gpu.py
relies on: every float64 reference agrees with float32 torch's own operator on the same inputs to 1e-5, the arg-max tie rows hold
exactly the ties they name, the large-logit rows are large, and nothing but a sliver at GroupNorm's ReLU kink is excluded."""
import pytest
import torch
import torch.nn.functional as F

import steve_kernel_cases as sc

AGREE = (1e-5, 1e-5)


def agrees(a32, ref64, what, keep=None):
    ratio = sc.err_over_bound(a32, ref64, AGREE, keep)
    print(f'{what}: float32 torch against the float64 reference, err / bound {ratio:.3f}')
    assert ref64.dtype == torch.float64
    assert ratio <= 1.0, (what, ratio)


def _torch_attention(c, H, causal):
    B, Lq, d = c['q'].shape
    qh, kh, vh = (t.view(B, -1, H, d // H).transpose(1, 2) for t in (c['q'], c['k'], c['v']))
    s = (qh @ kh.transpose(-1, -2)) * (d // H)**-0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Lq, Lq, dtype=torch.bool), 1), float('-inf'))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, d), torch.logsumexp(s, -1)


ATTN = ([(2, 3, hd, L, L, True) for L, hd in sc.FLASH_CASES + sc.GENERIC_CAUSAL_CASES] +
        [(3, 2, hd, Lq, Lk, False) for Lq, Lk, hd in sc.GENERIC_CROSS_CASES] + [(3, 2, hd, 1, Lk, False) for Lk, hd in sc.DECODE_CASES])


def test_attention_references():
    assert {hd for _, _, hd in sc.GENERIC_CROSS_CASES} == set(sc.HEAD_DIMS)
    for B, H, hd, Lq, Lk, causal in ATTN:
        c = sc.attention_case(B, H, hd, Lq, Lk, causal)
        out, lse = _torch_attention(c, H, causal)
        what = f'attention B {B} H {H} hd {hd} Lq {Lq} Lk {Lk} causal {causal}'
        agrees(out, c['out'], what)
        agrees(lse, c['lse'], what + ' lse')
        assert torch.isfinite(c['out']).all() and torch.isfinite(c['lse']).all() and 0 < c['smax'] < 20


def test_dispatch_tables_name_the_sizes_the_code_switches_at():
    """the thresholds of steve_decoder.hip, restated: a table that loses one of these sizes no longer covers its branch"""
    assert {127} <= set(sc.GENERIC_CAUSAL_L) and {128, 129} <= set(sc.FLASH_L)          # causal && Lq >= 128
    assert any(L % 64 not in (0, 1) and L > 128 for L in sc.FLASH_L)                    # full tile, then a ragged diagonal tile
    assert any(Lq > 256 for Lq, _, _ in sc.GENERIC_CROSS_CASES)                         # second workgroup in x
    assert {1, 64, 65, 256, 257} <= set(sc.DECODE_LK)
    assert {1024, 1028, 4096, 4100} <= set(sc.ROW_V) and any(V % 4 for V in sc.ROW_V)   # reg<1> | reg<4> | generic
    assert set(sc.LARGE_LOGIT_V) == {1024, 4096, 5000}
    for B, L, d, rows in sc.EMBED_CASES:
        assert (B * L * d // 4) % 256 != 0
    assert any(B * L * d // 4 < 256 for B, L, d, _ in sc.EMBED_CASES) and any(B * L * d // 4 > 256 for B, L, d, _ in sc.EMBED_CASES)
    n4 = [H * W * C // 4 for _, H, W, C, _ in sc.GN_SHAPES]
    assert sum(n < sc.GN_P for n in n4) == 2 and any(n % sc.GN_P for n in n4) and max(n4) == sc.GN_P * 256
    assert any(H != W and sh == 2 for _, H, W, _, sh in sc.GN_SHAPES)


@pytest.mark.parametrize('V', list(sc.ROW_V))
def test_row_references(V):
    for with_add, scale in sc.SOFTMAX_FORMS:
        c = sc.softmax_case(V, with_add, scale)
        z = (c['x'] + c['add'] if with_add else c['x']) * scale
        agrees(torch.softmax(z, -1), c['ref'], f'softmax V {V} add {with_add} scale {scale}')
        assert z.abs().max() <= 30.   # the premise of TOL_ROWS
    c = sc.softmax_case(V, False, 1.0, True)
    agrees(torch.log_softmax(c['x'], -1), c['ref'], f'log_softmax V {V}')
    for scale in (1.0, 10.0):
        c = sc.softmax_bwd_case(V, scale)
        t32 = torch._softmax_backward_data(c['dy'], c['y'], -1, torch.float32) * scale
        agrees(t32, c['ref'], f'softmax backward V {V} scale {scale}')
        assert (c['y'].sum(-1) - 1).abs().max() < 1e-5


@pytest.mark.parametrize('V', list(sc.LARGE_LOGIT_V))
def test_large_logit_rows_are_large(V):
    c = sc.large_logit_case(V)
    assert (c['zmax'] >= 250.).all() and (c['zmax'] <= 310.).all(), c['zmax']
    assert (c['x_log'].abs().max(-1)[0] >= 250.).all()
    # row 0: one dominant entry, the rest underflows; rows 3 and 4: a crowd next to the maximum, at +300 and at -300
    assert c['ref'][0].max() == 1.0 and (c['ref'][0] > 0.5).sum() == 1
    for r in (3, 4):
        assert (c['ref'][r] > 1e-3 * c['ref'][r].max()).sum() >= V // 4
    assert c['x'][3].min() > 25. and c['x'][4].max() < -25. and c['ref'][4].max() < 0.1
    e32 = sc.err_over_bound(c['t32'], c['ref'], sc.TOL_ROWS, per_row=True)
    e32_log = sc.err_over_bound(c['t32_log'], c['ref_log'], sc.TOL_ROWS, per_row=True)
    print(f'large logits V {V}: float32 torch err / bound, softmax {e32:.3f}, log_softmax {e32_log:.3f}')
    assert e32 > 0.5   # the rounding of z at |z| = 300 really shows: the fixed 1e-5 alone would not describe these rows


@pytest.mark.parametrize('V,R', sc.XENT_CASES)
def test_cross_entropy_reference(V, R):
    c = sc.xent_case(V, R)
    rows32 = F.cross_entropy(c['x'], c['tgt'], reduction='none')
    assert ((rows32.double() - c['rows']).abs() <= 1e-5 * c['rows'].abs() + 1e-6).all()
    assert abs(F.cross_entropy(c['x'], c['tgt']).item() - c['mean'].item()) <= 1e-5 * abs(c['mean'].item()) + 1e-6
    x, t = c['x'], c['tgt']
    if R == 1:
        assert t[0] == V - 1
    else:
        assert t[0] == 0 and t[1] == V - 1 and x[2, t[2]] == x[2].max()
        if V > 1:
            assert x[3].max() - x[3, t[3]] == 200. and abs(c['rows'][3].item() - 200.) < 20.


@pytest.mark.parametrize('V', sc.ARGMAX_V)
def test_argmax_tie_rows(V):
    c = sc.argmax_case(V)
    x, table = c['x'], c['table']
    assert x.dtype == torch.float32 and not torch.isnan(x).any()
    assert torch.equal(x.argmax(-1), c['expected'])          # torch.argmax: the first index of the maximum, 0 on an all -inf row
    for r, (what, ties, expected) in enumerate(table):
        top = torch.nonzero(x[r] == x[r].max())[:, 0].tolist()
        if ties is None:
            assert x[r].max() == sc.NEG_INF and top == list(range(V)) and expected == 0, what
        else:
            assert x[r].max() == sc.TIE_VALUE and top == sorted(set(ties)) and expected == min(ties), what
            if len(set(ties)) == 2:
                i, j = ties
                if 'one thread' in what:
                    assert (j - i) % 256 == 0, what
                elif 'lanes' in what:
                    assert i // 64 == j // 64 == 0 and i != j, what
                elif 'waves' in what:
                    assert (i % 256) // 64 != (j % 256) // 64, what
    assert (x[-1, :V - 1] == sc.NEG_INF).all() and x[-1, V - 1] > sc.NEG_INF and c['expected'][-1] == V - 1
    kinds = {w for w, _, _ in table}
    assert ('two waves' in kinds) == (V >= 131) and ('one thread, indices j and j + 256' in kinds) == (V >= 257)


@pytest.mark.parametrize('B,L,d,rows', sc.EMBED_CASES)
def test_embedding_reference(B, L, d, rows):
    c = sc.embed_case(B, L, d, rows)
    assert c['pos'].shape[0] == L and (c['idx'] == rows - 1).any() and (c['idx'] == 0).any() and c['idx'].max() < rows
    assert torch.equal(F.embedding(c['idx'], c['emb']) + c['pos'], c['ref']) and c['ref'].dtype == torch.float32


def _torch_groupnorm(c, relu, shuffle):
    y = F.group_norm(c['x'].permute(0, 3, 1, 2), 1, c['g'], c['b'], 1e-5)
    y = torch.relu(y) if relu else y
    return (F.pixel_shuffle(y, 2) if shuffle == 2 else y).permute(0, 2, 3, 1)


@pytest.mark.parametrize('F_,H,W,C,shuffle,relu', sc.GN_CASES)
def test_groupnorm_reference_and_kink(F_, H, W, C, shuffle, relu):
    c = sc.groupnorm_case(F_, H, W, C, shuffle, relu)
    assert c['ref'].shape == (F_, H * shuffle, W * shuffle, C // shuffle**2) == c['excluded'].shape
    frac = c['excluded'].double().mean().item()
    print(f'groupnorm {(F_, H, W, C)} shuffle {shuffle} relu {relu}: excluded at the kink {frac:.5f}')
    assert frac < 1e-3 and (relu or frac == 0.)
    agrees(_torch_groupnorm(c, relu, shuffle), c['ref'], 'groupnorm', ~c['excluded'])
    if relu:
        assert (c['ref'] == 0).double().mean() > 0.2 or H * W * C < 64   # the ReLU really cuts


@pytest.mark.parametrize('ratio', sc.GN_COND_RATIOS + (sc.GN_COND_LIMIT, ))
def test_groupnorm_conditioning_inputs(ratio):
    c = sc.groupnorm_case(*sc.GN_COND_SHAPE, 1, False, ratio)
    x = c['x'].double()
    assert abs(x.mean().item() / x.std().item() - ratio) < 0.05 * ratio and not c['excluded'].any()
    # float32 torch's own group_norm is held to 1e-5 at the small ratio only: at 8 and 32 it is the less accurate side (1.4 and 7.5
    # times the bound here), which is why the reference is float64
    t32 = _torch_groupnorm(c, False, 1)
    if ratio < 1:
        agrees(t32, c['ref'], f'groupnorm mean / std {ratio}')
    else:
        print(f'groupnorm mean / std {ratio}: float32 torch err / bound {sc.err_over_bound(t32, c["ref"], AGREE):.3f}')
