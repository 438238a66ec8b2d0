"""The rollout-unit plan of a pipelined run (slotformer_amd.pipeline.unit_sizes_for): a pure function of the batch counts, checked on the CPU.
The pipeline itself (streams, graphs, bit-identity of every plan with the serial calls) is tests/test_pipeline_gpu.py."""
import pytest

from slotformer_amd.pipeline import encode_lane_for, unit_sizes_for

C2_ROWS = 32 * 7 * 6      # token rows of a C2 batch (32 videos x 7 slots x 6 frames): 6 batches fill one round of row tiles
C5_ROWS = 64 * 6 * 8      # a C5 batch is more than a third of a round: units never grow


@pytest.mark.parametrize('n', list(range(0, 60)) + [100, 101, 203])
def test_sizes_cover_the_run(n):
    for rows in (C2_ROWS, C5_ROWS, 84):
        for G in (1, 2, 4, 7):
            for ramp in (False, True):
                sizes, n_tail = unit_sizes_for(n, G, rows, ramp=ramp)
                assert sum(sizes) == n and all(s >= 1 for s in sizes) and 0 <= n_tail <= len(sizes)
                if not ramp:
                    assert all(s * rows <= 8192 or s <= G for s in sizes)   # a unit grows beyond the group only within one round of row tiles
                    odd = [s for s in sizes if s != G]
                    assert len(odd) <= 2                                     # at most two units of another size (two unit objects per size)


def test_c2_plans():
    plan = lambda n, **k: unit_sizes_for(n, 4, C2_ROWS, **k)[0]  # noqa: E731
    assert plan(20) == [4, 4, 6, 6] and plan(21) == [4, 4, 4, 4, 5] and plan(22) == [4, 4, 4, 5, 5] and plan(23) == [4, 4, 4, 5, 6]
    assert plan(24) == [4, 4, 4, 6, 6] and plan(12) == [4, 4, 4] and plan(13) == [4, 4, 5] and plan(16) == [4, 6, 6]
    assert plan(100)[-2:] == [6, 6] and set(plan(100)[:-2]) == {4}
    # short runs and the opt-out keep the plain plan: full units + the remainder
    assert plan(11) == [4, 4, 3] and plan(5) == [4, 1] and plan(3) == [3] and plan(0) == []
    assert plan(21, spread=False) == [4, 4, 4, 4, 4, 1]
    # units that cannot grow (C5: a batch is 3072 rows) keep the remainder as a unit of its own
    assert unit_sizes_for(21, 4, C5_ROWS)[0] == [4, 4, 4, 4, 4, 1]
    # the ramp (off by default): the last batches in ever smaller units, which replace at most one full unit
    assert unit_sizes_for(20, 4, C2_ROWS, ramp=True) == ([4, 4, 4, 4, 2, 1, 1], 3)


# encode_lane_for: where every batch of a run is encoded.  (n_fill of a run of n, hybrid, hybrid_tail, n) -> the batches of the hybrid lane, worked by
# hand from the rule with two unmasked streams and two fill graphs: behind the fill every hybrid-th batch, none among the last hybrid_tail of the run
TOK_C2 = lambda n: dict(n=n, n_fill=min(18, n), hybrid=8, hybrid_tail=3)      # noqa: E731  (token-stationary C2: the fill is three units of 6 batches)
LANE_CASES = {
    'tok-C2-40': (TOK_C2(40), [25, 33]),
    'tok-C2-36': (TOK_C2(36), [25]),            # 33 + 3 is not < 36
    'tok-C2-20': (TOK_C2(20), []),
    'tok-C2-10': (TOK_C2(10), []),              # the fill covers the run
    'rows-C2-40': (dict(n=40, n_fill=12, hybrid=5, hybrid_tail=3), [16, 21, 26, 31, 36]),
}


def _lanes(n, n_fill, hybrid, hybrid_tail, free_streams=2, fill_par=2):
    return [encode_lane_for(j, n, n_fill, hybrid, hybrid_tail, free_streams, fill_par) for j in range(n)]


@pytest.mark.parametrize('case', sorted(LANE_CASES))
def test_encode_lanes(case):
    kw, hybrid_batches = LANE_CASES[case]
    n, n_fill = kw['n'], kw['n_fill']
    lanes = _lanes(**kw)
    assert [j for j, w in enumerate(lanes) if w == 'hybrid'] == hybrid_batches
    # batches below n_fill are 'fill', every other batch 'lane'
    assert all(w == ('fill' if j < n_fill else 'lane') for j, w in enumerate(lanes) if w != 'hybrid')
    assert all(j >= n_fill for j in hybrid_batches)
    if case == 'tok-C2-10':
        assert lanes == ['fill'] * 10
    plain = ['fill'] * n_fill + ['lane'] * (n - n_fill)
    assert _lanes(**dict(kw, hybrid=0)) == plain                       # hybrid = 0: no hybrid batch
    assert _lanes(**kw, free_streams=0) == plain                       # no free stream: no hybrid batch
    assert _lanes(**dict(kw, n_fill=0)) == ['lane'] * n                # no fill: no hybrid batch and no fill batch
