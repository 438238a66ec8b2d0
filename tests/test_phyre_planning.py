"""CPU: PHYRE planning without a device -- the float64 restatement of tests/phyre_readout_cases.py against the REFERENCE's own results
(tests/golden/phyre_readout.npz, tools/gen_golden_phyre_readout.py), the model's state-dict contract and factory, the no-CPU-fallback and
training-mode errors, every argument error of the C ABI (raised before any HIP call), the frame table of the planning driver, the host step of
AUCCESS against the reference's loop, and two properties of the seeded GPU inputs: no confidence near an accuracy threshold, no tie at c*."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import phyre_readout_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'phyre_readout.npz')
# float64 restatement vs the reference's float32 forward, of the largest |logit|: measured 5.2e-7 (profiles/phyre_planning.md); ten times that,
# far below 1e-4
RESTATEMENT_BOUND = 5e-6


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def test_float64_restatement_reproduces_the_reference(golden):
    rd, sd, slots, labels = cases.fixture_case()
    assert json.loads(str(golden['config']))['readout_dict'] == rd
    assert np.abs(cases.sin_pos_enc(len(rd['sel_slots']), rd['d_model']) - golden['enc_t_pe']).max() < 1e-6
    logits = cases.forward64(sd, rd, slots)
    d = rel_err(logits, golden['logits'])
    print(f'float64 restatement vs the reference fixture: {d:.3e} of the largest |logit|')
    assert d < RESTATEMENT_BOUND
    assert abs(cases.loss64(logits, labels) - float(golden['vqa_loss'])) < 1e-6 * abs(float(golden['vqa_loss']))
    assert json.loads(str(golden['acc_keys'])) == [f'acc_{t:.2f}' for t in cases.EVAL_THRESHS]
    acc = [cases.hits64(logits, labels, t).mean() for t in cases.EVAL_THRESHS]
    assert np.array_equal(np.float32(acc), golden['acc'])
    # the table is a frame table: sel_slots spelled out gives the same logits, a zero frame does not
    assert np.array_equal(cases.forward64(sd, rd, slots, [0, 3]), logits)
    assert rel_err(cases.forward64(sd, rd, slots, [-1, 3]), logits) > 1e-3


def test_state_dict_contract(golden):
    from slotformer_amd.phyre_planning.models import PHYREReadout
    want = json.loads(str(golden['state_dict_keys']))
    m = PHYREReadout()
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == want
    assert want == [[k, list(s)] for k, s in cases.state_shapes(cases.readout_dict())]
    assert np.abs(sd['enc_t_pe'].numpy() - golden['enc_t_pe']).max() < 1e-6 and not m.enc_t_pe.requires_grad
    cfg = json.loads(str(golden['config']))
    m = PHYREReadout(cfg['readout_dict'])
    assert (m.num_slots, m.slot_size, m.sel_slots, m.T) == (8, 128, [0, 3], 2)
    assert m.dtype == torch.float32 and m.device.type == 'cpu' and m.shape_ok()
    m.load_state_dict(cases.seeded_weights(cfg['readout_dict'], 1))   # (strict: every key, every shape)


class _Params:
    model = 'PHYREReadout'
    readout_dict = cases.readout_dict(N=7, sel=(0, 2, 4))


def test_build_model_through_both_packages():
    import slotformer_amd.phyre_planning as native
    alias = importlib.import_module('slotformer.phyre_planning')
    assert alias is native
    from slotformer.phyre_planning.models import PHYREReadout
    for pkg in (native, alias):
        m = pkg.build_model(_Params())
        assert isinstance(m, PHYREReadout) and m.num_slots == 7 and m.T == 3
    for name in ('PhysionReadout', 'PhyreReadout'):
        nope = _Params()
        nope.model = name
        with pytest.raises(NotImplementedError):
            native.build_model(nope)
    with pytest.raises(NotImplementedError):
        native.build_dataset(_Params())
    with pytest.raises(NotImplementedError):
        native.build_method()
    assert (native.INVALID_INPUT, native.NOT_SOLVED) == (0, -1) and native.SOLVED > 0


def test_no_cpu_fallback_training_mode_and_unsupported_shapes():
    from slotformer_amd import harness, ops, phyre_planning
    from slotformer_amd.phyre_planning.models import PHYREReadout
    m = PHYREReadout()
    slots = torch.zeros(2, 4, 8, 128)
    assert m.training
    with pytest.raises(NotImplementedError, match='training kernels of this readout .* not built'):
        m({'slots': slots})
    m.eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m({'slots': slots})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_train_loss({'label': torch.zeros(2)}, {'logits': torch.zeros(2)})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_eval_loss({'label': torch.zeros(2)}, {'logits': torch.zeros(2)})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harness.phyre_plan(None, None, m, torch.zeros(2, 1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.phyre_auccess_ranks(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            phyre_planning.auccess(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32))
    # an uncovered readout_dict constructs and loads, and is refused with the limits at first use
    for odd in (dict(num_slots=17), dict(slot_size=100), dict(d_model=256, ffn_dim=1024), dict(num_heads=4), dict(num_layers=9), dict(norm_first=False),
                dict(sel_slots=list(range(12))), dict(t_pe='')):
        rd = dict(cases.READOUT_DICT, **odd)
        o = PHYREReadout(rd).eval()
        o.load_state_dict(o.state_dict())
        assert not o.shape_ok(), odd
        with pytest.raises(NotImplementedError, match='multiple of 32'):
            o({'slots': torch.zeros(1, 12, rd['num_slots'], rd['slot_size'])})
    assert ops.phyre_readout_ok(8, 128, 2) and ops.phyre_readout_ok(1, 32, 1, num_layers=1) and ops.phyre_readout_ok(16, 256, 5, num_layers=8)
    assert ops.phyre_readout_ok(1, 32, 95) and not ops.phyre_readout_ok(1, 32, 96)       # 96 tokens, 97 tokens
    assert ops.phyre_readout_ok(5, 64, 19) and not ops.phyre_readout_ok(8, 128, 12)      # 96 tokens, 97 tokens
    for bad in ((0, 128, 2), (17, 128, 2), (8, 100, 2), (8, 288, 2), (8, 0, 2), (8, 128, 0)):
        assert not ops.phyre_readout_ok(*bad), bad
    for kw in (dict(d_model=256), dict(num_heads=4), dict(ffn=1024), dict(num_layers=0), dict(num_layers=9)):
        assert not ops.phyre_readout_ok(8, 128, 2, **kw), kw


def test_abi_argument_errors():
    """Negative return codes with a message that names the limits, before any HIP call."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)
    layers = (_lib.sf_tfm_layer * 8)()
    for l in layers:
        l.tok_packed = 16
    unpacked = (_lib.sf_tfm_layer * 8)()

    def err():
        return lib.sf_last_error_string().decode()

    def fwd(slots=one, N=8, Cc=128, T=2, sel=(0, 3), T_all=4, nl=4, shape=(128, 8, 512), st=8 * 128, B=4, V=4, vidx=None, lay=layers, ws=one,
            ws_bytes=1 << 30, table=None, sidx=None, slen=0, logits=one):
        sel_arr = (C.c_int * max(len(sel), 1))(*sel) if sel is not None else None
        return lib.sf_phyre_readout_fwd_f32(slots, T_all * st, st, V, T_all, vidx, sel_arr, one, one, one, one, lay, nl, *shape, one, one, one, one, logits,
                                            None, sidx, table, slen, B, T, N, Cc, ws, ws_bytes, None)

    old = lib.sf_get_precision()
    lib.sf_set_precision(1)
    try:
        for kw in (dict(slots=None), dict(sel=None), dict(lay=None), dict(ws=None), dict(logits=None)):
            assert fwd(**kw) < 0 and 'null pointer' in err(), kw
        for kw in (dict(N=0), dict(N=17), dict(Cc=100), dict(Cc=288), dict(Cc=0), dict(T=0, sel=()), dict(T=12, sel=(0, ) * 12),
                   dict(shape=(256, 8, 1024)), dict(shape=(128, 4, 512)), dict(shape=(128, 8, 256)), dict(nl=0), dict(nl=9)):
            assert fwd(**kw) < 0 and 'unsupported shape' in err() and '1 + T * num_slots <= 96' in err() and '(128, 8, 512)' in err(), kw
        assert fwd(B=0) < 0 and 'B >= 1' in err()
        assert fwd(st=8 * 128 - 4) < 0 and 'frame stride' in err()
        assert fwd(st=8 * 128 + 2) < 0 and 'frame stride' in err()
        assert fwd(B=5) < 0 and 'without a video_index' in err()
        for sel in ((0, 4), (-2, 1)):
            assert fwd(sel=sel) < 0 and 'sel[t] must lie in [-1, T_all)' in err(), sel
        assert fwd(table=one, sidx=None, slen=4) < 0 and 'scatter' in err()
        assert fwd(table=one, sidx=one, slen=0) < 0 and 'scatter' in err()
        assert fwd(slots=C.c_void_p(20)) < 0 and '16-byte aligned' in err()
        need = lib.sf_phyre_readout_workspace_bytes(4, 8, 2)
        assert need == 2 * 4 * 17 * 128 * 4
        assert fwd(ws_bytes=need - 1) < 0 and 'workspace too small' in err()
        assert fwd(lay=unpacked) < 0 and 'tok_packed' in err()
        # the layers exist in split-bf16 only: another process precision is an error, not another path
        lib.sf_set_precision(0)
        assert fwd() < 0 and 'split-bf16 mode only' in err()
        lib.sf_set_precision(2)
        assert fwd() < 0 and 'split-bf16 mode only' in err()
    finally:
        lib.sf_set_precision(old)
    assert lib.sf_phyre_readout_workspace_bytes(0, 8, 2) == 0 and lib.sf_phyre_readout_workspace_bytes(4, 17, 2) == 0
    assert lib.sf_phyre_readout_workspace_bytes(4, 8, 12) == 0
    assert lib.sf_phyre_readout_ok(8, 128, 2, 128, 8, 512, 4) == 1 and lib.sf_phyre_readout_ok(8, 128, 2, 128, 8, 512, 9) == 0
    assert lib.sf_phyre_auccess_f32(None, one, one, 1, 1, None) < 0 and 'null pointer' in err()
    assert lib.sf_phyre_auccess_f32(one, one, one, 0, 5, None) < 0 and 'tasks >= 1' in err()
    assert lib.sf_phyre_auccess_f32(one, one, one, 2, 0, None) < 0 and 'actions >= 1' in err()


def test_frame_table_of_the_planning_driver():
    from slotformer_amd.phyre_planning import frame_table
    # rollout-buffer frames [slot0, pred_0, pred_1, ...]: the reference classifies cat(padded zero frames, predictions)
    assert frame_table([0, 3]) == [-1, 1]
    assert frame_table([0, 3], reference_indexing=False) == [0, 3]
    assert frame_table([3, 0]) == [1, -1]
    assert frame_table([0, 2, 4]) == [-1, -1, 1]
    assert frame_table([4, 4]) == [1, 1]
    # against the concatenation itself: frame numbers as values
    for sel in ([0, 3], [1, 5, 2], [7]):
        vid_len = max(sel) + 1
        buf = np.arange(vid_len)                                 # buffer frame f holds the value f (0: slot0, f: prediction f - 1)
        cat = np.concatenate([np.full(vid_len - 1, -1), buf[1:]])   # gt_slots = the padded zeros (-1), pred_slots
        assert frame_table(sel) == [int(cat[s]) for s in sel]
    with pytest.raises(ValueError):
        frame_table([])
    with pytest.raises(ValueError):
        frame_table([-1, 2])


def test_auccess_host_step_against_the_reference_loop():
    from slotformer_amd.phyre_planning import auccess_from_ranks
    for name, (conf, status) in cases.auccess_cases().items():
        if name == 'tie':
            continue
        ref_auccess, ref_rate, ref_table, ref_first = cases.auccess_reference(conf, status)
        out = auccess_from_ranks(ref_first, actions=conf.shape[1])
        assert np.array_equal(out['success_rate'], ref_rate), name
        assert out['auccess'] == pytest.approx(ref_auccess, rel=1e-12, abs=1e-12), name
        assert np.array_equal(out['first_rank'], ref_first)
        assert np.array_equal(ref_first[:, None] < np.arange(1, 101)[None, :], ref_table > 0), name
    # closed forms: the first attempt always solves -> 100; never -> 0; a task without a solved action and fewer than 100 actions stays at 0
    assert auccess_from_ranks([0, 0])['auccess'] == pytest.approx(100.0)
    assert auccess_from_ranks([100, 5000])['auccess'] == 0.0
    assert auccess_from_ranks([7], actions=7)['auccess'] == 0.0
    w = np.log(np.arange(2, 102)) - np.log(np.arange(1, 101))
    assert auccess_from_ranks([0, 100])['auccess'] == pytest.approx(50.0)
    assert auccess_from_ranks([1])['auccess'] == pytest.approx(100.0 * w[1:].sum() / w.sum())
    with pytest.raises(ValueError):
        auccess_from_ranks([])


def test_seeded_gpu_cases_stay_clear_of_the_accuracy_thresholds():
    """The exact-count tests on the device hold only if no float64 confidence lies within the device tolerance of a threshold."""
    rd, sd, slots, _ = cases.fixture_case()
    seen = [('fixture', cases.forward64(sd, rd, slots))]
    for case in cases.FORWARD_CASES:
        rd, sd, slots, table = cases.forward_case(case)
        seen.append((case['name'], cases.forward64(sd, rd, slots, table, case.get('video_index'))))
    assert len(seen) == 1 + len(cases.FORWARD_CASES)
    for name, logits in seen:
        clear, need = cases.threshold_clearance(logits), cases.THRESH_MARGIN(logits)
        print(f'{name}: min |sigmoid(logit) - threshold| = {clear:.4f}, needed {need:.4f}')
        assert clear > need, name


def test_auccess_cases_have_no_tie_at_the_best_solved_confidence():
    all_cases = cases.auccess_cases()
    assert set(all_cases) == {'three-tasks', 'first-and-last', 'tie'}
    for name, (conf, status) in all_cases.items():
        assert conf.dtype == np.float32 and status.dtype == np.int32 and conf.shape == status.shape
        ties = 0
        for c, s in zip(conf, status):
            if (s > 0).any():
                cstar = c[s > 0].max()
                ties += int(((c == cstar) & (s != 0)).sum() > 1)
        assert ties == (1 if name == 'tie' else 0), name
    conf, status = all_cases['three-tasks']
    assert conf.shape == (3, 257) and (status == 0).any(1).all() and not (status[1] > 0).any() and 0 < (status[2] != 0).sum() < 100
    assert (status[2] > 0).any()
