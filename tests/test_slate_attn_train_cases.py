"""The table and the references of tests/slate_attn_train_cases.py, held on the CPU to what tests/test_slate_attn_train_gpu.py relies
on: the float64 reference computed by autograd and the one computed from the kernels' closed form agree to 1e-12, the table reaches
every kernel in each precision mode and every edge it names, the dropout indices fit 32 bits, the p = 0.5 cases do hold fully
dropped rows, and a plain float32 evaluation of every case stays below a tenth of the exact-f32 bound (so a miss on the device is
the kernel's, not the inputs')."""
import pytest
import torch

import slate_attn_train_cases as tc
import steve_kernel_cases as sc

IDS = [tc.case_id(c) for c in tc.CASES]


@pytest.mark.parametrize('c', tc.CASES, ids=IDS)
def test_the_two_references_agree(c):
    """autograd against the closed form, 1e-12 relative to the largest element of each output"""
    ref = tc.reference64(c)
    for name in ('out', 'lse', 'dq', 'dk', 'dv'):
        a, b = ref['closed'][name], ref[name]
        assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.isfinite(b).all(), name
        err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), tc.floor_base(c, name) or 0.)
        assert scale > 1e-3 and err <= 1e-12 * scale, (name, err, scale)
    d = c.H * c.hd
    assert ref['out'].shape == ref['dq'].shape == (c.B, c.Lq, d) and ref['dk'].shape == ref['dv'].shape == (c.B, c.Lk, d)
    assert ref['lse'].shape == (c.B, c.H, c.Lq) and 0 < ref['smax'] < 20


@pytest.mark.parametrize('c', tc.CASES, ids=IDS)
def test_float32_on_the_cpu_is_far_inside_the_bound(c):
    """input sanity: float32 torch on the CPU against float64, at most 0.1 of the exact-f32 bound on every output"""
    ref = tc.reference64(c)
    t32 = tc.attention(ref['q'], ref['k'], ref['v'], ref['g'], c, torch.float32)
    worst = max(tc.ratio(t32[n], ref[n], sc.TOL['f32'], tc.floor_base(c, n)) for n in ('out', 'dq', 'dk', 'dv'))
    lse = (t32['lse'].double() - ref['lse']).abs().max().item() / (sc.TOL['f32'][0] * ref['smax'] + sc.TOL['f32'][1])
    print(f'{tc.case_id(c)}: float32 torch err / bound {worst:.4f}, lse {lse:.4f}')
    assert worst <= 0.1 and lse <= 0.1, (worst, lse)


def test_sizes_stay_small_and_indices_fit_32_bits():
    for c in tc.CASES:
        assert c.B * c.H * c.Lq * c.Lk < 2**32
        assert c.p in (0., 0.1, 0.5) and (not c.causal or c.Lq == c.Lk) and isinstance(c.edge, str) and c.edge
        if c is not tc.WORKLOAD:
            assert c.B <= 3 and c.H <= 3 and max(c.Lq, c.Lk) <= 257
    assert sum(max(c.Lq, c.Lk) > 257 for c in tc.CASES) == 1
    w = tc.WORKLOAD
    assert (w.B, w.H, w.hd, w.Lq, w.causal, w.p) == (1, 1, 48, 1025, True, 0.1)


def test_every_kernel_is_reached_in_each_mode():
    for mode in tc.MODES:
        for causal in (True, False):
            for p in (0., 0.1):
                got = {tc.bwd_kernel_of(c.hd, mode, c.H * c.hd, c.H * c.hd) for c in tc.BWD_CASES if c.causal == causal and c.p == p}
                assert got == ({'bwd<32>', 'bwd48v2', 'bwd<64>'} if mode == 'bf16x3' else {'bwd<32>', 'bwd<64>'}), (mode, causal, p, got)
                fwd = {tc.fwd_kernel_of(c.hd, c.Lq, c.causal, mode) for c in tc.CASES if c.causal == causal and c.p == p}
                flash = {'flash_bf3<TRAIN>' if mode == 'bf16x3' else 'flash<TRAIN>'} if causal else set()
                assert fwd == {'fwd_train<32>', 'fwd_train<64>'} | flash, (mode, causal, p, fwd)
        # the 48-wide cases run the 64-wide kernel in exact f32, and with k or v off 16 bytes in either mode
        for hd in tc.HD_W48:
            assert tc.bwd_kernel_of(hd, 'bf16x3', 96, 96) == 'bwd48v2' and tc.bwd_kernel_of(hd, 'f32', 96, 96) == 'bwd<64>'
            assert tc.bwd_kernel_of(hd, 'bf16x3', 98, 96) == tc.bwd_kernel_of(hd, 'bf16x3', 96, 96, kv_aligned=False) == 'bwd<64>'
        assert set(tc.TOL_BWD) >= {(tc.bwd_kernel_of(c.hd, mode, 4, 4), mode) for c in tc.BWD_CASES}
        assert set(tc.TOL_FWD) >= {(tc.fwd_kernel_of(c.hd, c.Lq, c.causal, mode), mode) for c in tc.CASES}
    assert tc.bwd_kernel_of(18, 'f32', 36, 36) is None and tc.fwd_kernel_of(18, 9, True, 'f32') == 'fwd_train<32>'
    assert tc.fwd_kernel_of(3, 9, True, 'f32') is None and tc.fwd_kernel_of(66, 9, True, 'f32') is None
    assert tc.fwd_kernel_of(48, 127, True, 'f32') == 'fwd_train<64>' and tc.fwd_kernel_of(48, 128, True, 'f32') == 'flash<TRAIN>'
    assert tc.fwd_kernel_of(48, 257, False, 'f32') == 'fwd_train<64>' and tc.fwd_kernel_of(50, 193, True, 'bf16x3') == 'fwd_train<64>'


def test_the_covering_design_holds():
    bwd, everything = tc.BWD_CASES, tc.CASES
    assert {c.hd for c in bwd} == set(tc.BWD_HEAD_DIMS) == {4, 12, 16, 28, 32, 36, 40, 44, 48, 52, 60, 64}
    assert {c.hd for c in everything if not c.bwd} == set(tc.HD_FWD_ONLY) == {2, 18, 50}
    assert set(tc.CAUSAL_L) == {1, 2, 63, 64, 65, 127, 128, 129, 191, 193}
    assert set(tc.CROSS) == {(2, 1), (1, 33), (70, 6), (64, 7), (65, 64), (130, 65), (129, 128), (257, 130)}
    # every head dim meets a ragged causal length and a cross shape
    for hd in tc.BWD_HEAD_DIMS + tc.HD_FWD_ONLY:
        assert any(c.hd == hd and c.causal and c.Lq % 64 for c in everything), hd
        assert any(c.hd == hd and not c.causal for c in everything), hd
    # every length and every cross shape meets hd 48 and one head dim of each generic width, at p = 0
    for causal, shapes in ((True, [(L, L) for L in tc.CAUSAL_L]), (False, list(tc.CROSS))):
        for Lq, Lk in shapes:
            hds = {c.hd for c in bwd if (c.causal, c.Lq, c.Lk, c.p) == (causal, Lq, Lk, 0.)}
            assert 48 in hds and hds & set(tc.HD_W32) and hds & set(tc.HD_W64), (causal, Lq, Lk, hds)
    # p = 0 everywhere: every (shape, head dim) that occurs with dropout occurs without, but for the one long case
    for c in everything:
        if c.p > 0 and c is not tc.WORKLOAD and c not in (tc.DROPPED_CAUSAL, tc.DROPPED_CROSS) and c.bwd:
            assert any((o.causal, o.Lq, o.Lk, o.p) == (c.causal, c.Lq, c.Lk, 0.) for o in everything), c
    assert tc.DROPPED_CAUSAL in everything and tc.DROPPED_CROSS in everything and tc.WORKLOAD in everything
    d = tc.DROPPED_CAUSAL, tc.DROPPED_CROSS
    assert (d[0].B, d[0].H, d[0].hd, d[0].Lq, d[0].causal, d[0].p) == (2, 2, 4, 65, True, 0.5)
    assert (d[1].B, d[1].H, d[1].Lq, d[1].Lk, d[1].causal, d[1].p) == (3, 2, 70, 6, False, 0.5)
    for c in tc.LAYOUT_CAUSAL + tc.LAYOUT_CROSS + [tc.CROSS_NODE]:
        assert c in bwd
    for group in (tc.LAYOUT_CAUSAL, tc.LAYOUT_CROSS):
        assert {tc.bwd_kernel_of(c.hd, 'bf16x3', 4, 4) for c in group} == {'bwd<32>', 'bwd48v2', 'bwd<64>'}


def test_every_named_edge_is_reached():
    w48 = [c for c in tc.BWD_CASES if c.hd in tc.HD_W48]
    blocks = lambda n: (n + 63) // 64   # noqa: E731

    def pairs(c):
        return [(qb, kb) for kb in range(blocks(c.Lk)) for qb in range(kb if c.causal else 0, blocks(c.Lq))]
    # `full` next to a ragged last query block, causal and cross; a `full` pair at k0 + 64 == Lk exactly; a pair that is not `full`
    # only because of its keys
    for causal in (True, False):
        assert any(c.Lq % 64 and any(tc.is_full(c.Lq, c.Lk, c.causal, *p) for p in pairs(c)) for c in w48 if c.causal == causal)
    assert any(tc.is_full(c.Lq, c.Lk, c.causal, qb, kb) and kb * 64 + 64 == c.Lk for c in w48 for qb, kb in pairs(c))
    assert any(not c.causal and qb * 64 + 64 <= c.Lq and kb * 64 + 64 > c.Lk for c in w48 for qb, kb in pairs(c))
    c193 = tc.find(True, 193, 193, 48, 0.)
    assert [p for p in pairs(c193) if tc.is_full(193, 193, True, *p)] == [(1, 0), (2, 0), (2, 1)]
    # with dropout: clamped rows and keys are hashed in a block that is not `full`, and a `full` block is hashed too
    for c in (tc.find(True, 193, 193, 48, 0.1), tc.find(False, 257, 130, 48, 0.1), tc.find(True, 191, 191, 40, 0.1)):
        kinds = {tc.is_full(c.Lq, c.Lk, c.causal, *p) for p in pairs(c)}
        assert kinds == {True, False} and (c.Lq % 64 and c.Lk % 64), c
    for kernel_hds in (tc.HD_W32, tc.HD_W48, tc.HD_W64):
        mine = [c for c in tc.BWD_CASES if c.hd in kernel_hds]
        assert any(c.Lq == 1 and c.causal for c in mine) and any(c.Lk == 1 and not c.causal for c in mine)
        assert any(c.Lq == 1 and not c.causal for c in mine)
        assert {63, 64, 65} <= {c.Lq for c in mine if c.causal}
        assert any(c.Lk % 64 == 1 and c.Lk > 64 for c in mine) and any(c.Lq % 64 == 1 and c.Lq > 64 for c in mine)
        assert {127, 128, 129} <= {c.Lq for c in mine if c.causal}
    # zero-padded head dims of every width
    assert {4, 12, 16, 28} <= {c.hd for c in tc.BWD_CASES} and {36, 40, 44} <= {c.hd for c in w48} and {52, 60} <= {c.hd for c in tc.BWD_CASES}


@pytest.mark.parametrize('c', [tc.DROPPED_CAUSAL, tc.DROPPED_CROSS], ids=tc.case_id)
def test_half_dropout_drops_whole_rows(c):
    """a row whose live keys are all dropped: out = 0 and no gradient through it, but lse is still the row's log-sum-exp"""
    n = tc.fully_dropped_rows(c)
    print(f'{tc.case_id(c)}: {n} fully dropped rows')
    assert n >= 1
    ref = tc.reference64(c)
    gone = ((tc.keep_mask(c) & tc.live_mask(c)).sum(-1) == 0)                   # [B, H, Lq]
    out = ref['out'].view(c.B, c.Lq, c.H, c.hd).transpose(1, 2)[gone]
    dq = ref['dq'].view(c.B, c.Lq, c.H, c.hd).transpose(1, 2)[gone]
    assert (out == 0).all() and (dq == 0).all() and torch.isfinite(ref['lse'][gone]).all()


def test_node_cases():
    c = tc.SELF_NODE
    assert (c.causal, c.Lq, c.p) == (True, 129, 0.1) and tc.bwd_kernel_of(c.hd, 'bf16x3', 3 * c.H * c.hd, 3 * c.H * c.hd) == 'bwd48v2'
    n = tc.self_attention_node_case()
    assert n['out'].dtype == torch.float64 and all(torch.isfinite(t).all() for t in [n['out'], n['dx']] + n['dw'])
    assert 0.5 < (n['x'].double() @ n['w'][0].double().t()).std() < 2.
    c = tc.CROSS_NODE
    assert not c.causal and c.p == 0.1 and c.Lq % 64 and c.Lk % 64
