"""CPU: 9 .. 16 slots.  The argument checks of the C ABI (which run before any device work), the oracle against the fixtures of
tools/gen_golden_slots16.py (outputs of the reference's own classes at 9, 11 and 16 slots), and the pipeline's unit plan at 11 and 16 slots.
The kernels themselves: tests/test_slots16_gpu.py."""
import ctypes as C

import pytest

import slots16_cases as sc
import test_oracle_golden as tog

ONE = C.c_void_p(16)   # a non-null dummy pointer: every call below returns before it is dereferenced (B = 0, or a rejected argument)


def _err(lib):
    return lib.sf_last_error_string().decode()


def test_iteration_entry_points_take_16_slots():
    from slotformer_amd import _lib
    lib = _lib.lib()
    for D, HW in ((128, 4096), (256, 256), (64, 80)):
        assert lib.sf_slot_attn_iter_f32(ONE, ONE, D, HW * D, ONE, ONE, ONE, None, 0, HW, 16, D, 0.1, 1e-6, None) == 0
        assert lib.sf_slot_attn_iter_f32(ONE, ONE, D, HW * D, ONE, ONE, ONE, None, 0, HW, 9, D, 0.1, 1e-6, None) == 0
        assert lib.sf_slot_attn_iter_f32(ONE, ONE, D, HW * D, ONE, ONE, ONE, None, 0, HW, 17, D, 0.1, 1e-6, None) < 0
        assert '16' in _err(lib)
    assert lib.sf_slot_attn_iter_f32(ONE, ONE, 128, 4096 * 128, ONE, ONE, ONE, None, 0, 4096, 0, 128, 0.1, 1e-6, None) < 0
    assert lib.sf_slot_attn_iter_bf16(ONE, ONE, 128, 4096 * 128, ONE, ONE, ONE, None, 0, 4096, 16, 128, 0.1, 1e-6, None) == 0
    assert lib.sf_slot_attn_iter_bf16(ONE, ONE, 128, 4096 * 128, ONE, ONE, ONE, None, 0, 4096, 17, 128, 0.1, 1e-6, None) < 0
    assert '16' in _err(lib)


def test_backward_entry_points_split_at_8_slots():
    """sf_slot_attn_iter_bwd_f32 keeps its 8-slot contract (tests/test_abi.py); the 9 .. 16-slot form has its own entry point and workspace query
    with the same signature."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    assert _lib.SIGNATURES['sf_slot_attn_iter_bwd16_f32'] == _lib.SIGNATURES['sf_slot_attn_iter_bwd_f32']
    assert _lib.SIGNATURES['sf_slot_attn_iter_bwd16_workspace_bytes'] == _lib.SIGNATURES['sf_slot_attn_iter_bwd_workspace_bytes']

    def call(fn, B, N, D=128):
        return fn(ONE, ONE, D, 4096 * D, ONE, ONE, ONE, 1, ONE, ONE, ONE, 0, ONE, B, 4096, N, D, 0.1, 1e-6, ONE, 1 << 30, None)

    assert call(lib.sf_slot_attn_iter_bwd16_f32, 0, 16) == 0 and call(lib.sf_slot_attn_iter_bwd16_f32, 0, 9) == 0
    assert call(lib.sf_slot_attn_iter_bwd16_f32, 0, 8) == 0
    assert call(lib.sf_slot_attn_iter_bwd16_f32, 0, 17) < 0 and '16' in _err(lib)
    assert call(lib.sf_slot_attn_iter_bwd16_f32, 0, 16, D=100) < 0 and 'slot_size' in _err(lib)
    assert call(lib.sf_slot_attn_iter_bwd_f32, 1, 9) < 0 and '<= 8' in _err(lib)     # rejected before any device work, as before
    assert call(lib.sf_slot_attn_iter_bwd_f32, 0, 9) < 0
    assert call(lib.sf_slot_attn_iter_bwd_f32, 0, 8) == 0
    for N in (1, 7, 8, 9, 16):
        assert lib.sf_slot_attn_iter_bwd16_workspace_bytes(3, 4096, N, 128) == lib.sf_slot_attn_iter_bwd_workspace_bytes(3, 4096, N, 128) > 0


def test_training_workspace_query_takes_16_slots():
    from slotformer_amd import _lib
    lib = _lib.lib()
    m = _lib.sf_slot_attention()
    m.in_features, m.slot_size, m.mlp_hidden = 128, 128, 256
    sizes = {}
    for N in (7, 8, 9, 16, 17):
        m.num_slots = N
        sizes[N] = lib.sf_slot_attention_train_workspace_bytes(C.byref(m), 2, 1024, 2)
    assert sizes[16] > sizes[9] > sizes[8] > sizes[7] > 0 and sizes[17] == 0


def test_tile16_switch_round_trips():
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_slot_attn_tile16()
    assert old == 1
    assert lib.sf_set_slot_attn_tile16(0) == 0 and lib.sf_get_slot_attn_tile16() == 0
    assert lib.sf_set_slot_attn_tile16(old) == 0 and lib.sf_get_slot_attn_tile16() == old


def test_encode_workspace_grows_with_the_slots_only_in_the_slot_rows():
    """The encode workspace at 11 and 16 slots: every carve that depends on N is linear in it (slot rows, partial records, predictor rows), so the
    sizes at 8, 12 and 16 slots lie on one line -- and the queries answer (non-zero) for 16 slots."""
    from slotformer_amd import _lib, configs
    from test_encode_plan import encoder
    lib = _lib.lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(1)
    try:
        for kw in (dict(kernel_mlp=True, pred='transformer', rnn=True), dict(kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01')):
            by_n = {}
            for N in (8, 12, 16):
                m = encoder(configs.savi_cfg(64, N, **kw))
                by_n[N] = [lib.sf_savi_encode_workspace_bytes(C.byref(m), 32), lib.sf_savi_encode_fork_workspace_bytes(C.byref(m), 32, 6),
                           lib.sf_savi_encode_batched_workspace_bytes(C.byref(m), 32, 6)]
            for a, b, c in zip(by_n[8], by_n[12], by_n[16]):
                assert 0 < a < b < c and abs((c - b) - (b - a)) <= 3 * 4096   # (256-byte rounding of the ~30 carves)
    finally:
        lib.sf_set_precision(old)


@pytest.mark.parametrize('name', list(sc.SAVI_CASES))
def test_oracle_savi(name):
    cfg, kw = sc.SAVI_CASES[name]
    tog.test_savi(name, cfg, kw['B'], kw['T'], kw['seed'], kw.get('noise_seed'))


@pytest.mark.parametrize('name', list(sc.ROLL_CASES))
def test_oracle_rollout(name):
    cfg, kw = sc.ROLL_CASES[name]
    tog.test_rollout(name, cfg, kw['B'], kw['pred_len'], kw['seed'], False)


@pytest.mark.parametrize('name', list(sc.SAVI_TRAIN_CASES))
def test_oracle_savi_training_step(name):
    cfg, kw = sc.SAVI_TRAIN_CASES[name]
    assert kw['B'] == 1
    tog.test_oracle_savi_training_step_matches_reference(name, sc.register(cfg), kw['T'], kw['seed'], kw['noise_seed'], 1e-4)


# ---- the pipeline's unit plan ----
def _rollouter(N, hist=6):
    import golden_util as gu
    from slotformer_amd.video_prediction.models import SlotRollouter
    return SlotRollouter(**gu.rollout_cfg(N, 128, hist, 256, 4, 8, 1024)['rollout_dict']).eval()


@pytest.mark.parametrize('N', [11, 16])
def test_unit_plan_stays_within_its_row_limits(N, monkeypatch):
    """pipeline.unit_batches_for / unit_sizes_for / encode_group_for at 11 and 16 slots: a unit beyond the default of 4 batches stays within one
    round of row tiles (8192 token rows); the plan of a run covers the run.  (The rule asks the
    library whether the rollouter runs the fused layers -- batch-size independent results; answered 'yes' here, as on the GPU for this shape.)"""
    from slotformer_amd import _lib, pipeline
    monkeypatch.setattr(_lib.lib(), 'sf_rollout_is_fused', lambda p: 1, raising=False)
    roll = _rollouter(N)
    T = 6
    seen = set()
    for batch in (1, 2, 4, 5, 14, 16, 32, 64):
        rows = batch * N * T
        for n in (1, 2, 9, 10, 12, 20, 21, 29, 39, 40, 41, 84, 100):
            g = pipeline.unit_batches_for(roll, batch, n, T)
            seen.add(g)
            assert g is None or (5 <= g <= n and g * rows <= 8192)
            sizes, n_tail = pipeline.unit_sizes_for(n, g or 4, rows)
            assert sum(sizes) == n and all(s >= 1 and (s * rows <= 8192 or s <= (g or 4)) for s in sizes)
            e = pipeline.encode_group_for(batch, n)
            assert 1 <= e <= max(1, 32 // batch) and n % e == 0
    assert seen - {None}   # (the rule did pick larger units for some run)


@pytest.mark.parametrize('N,hist,vpw', [(11, 6, 1), (16, 6, 1), (16, 5, 1), (9, 6, 2), (16, 1, 8)])
def test_videos_per_token_workgroup(N, hist, vpw):
    """The token-stationary window holds at most 96 tokens; a 128-token workgroup owns 128 // (N * hist) whole videos: 1 at 16 x 6 = 96 tokens, the
    window limit, and never 0 within it."""
    assert N * hist <= 96 and 128 // (N * hist) == vpw >= 1
    from slotformer_amd import pipeline
    assert pipeline.tok_unit_batches(_rollouter(N, hist), 32, hist) is None   # (a host rollouter: no token-stationary units)
