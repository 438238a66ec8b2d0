"""CPU: the Physion VQA readout without a device -- the float64 restatements of tests/physion_readout_cases.py against the REFERENCE's own results
(tests/golden/physion_readout.npz, tools/gen_golden_physion_readout.py), the model's state-dict contract and factory, the argument errors of the C
ABI (raised before any HIP call), the no-CPU-fallback rule, the batch schedule of `fit`, and the split-bf16 emulation's distance from float64 for
every seeded case of the GPU tests."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import physion_readout_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'physion_readout.npz')
EMULATION_BOUND = 2.5e-4   # of the largest |logit|: four times it stays under the project's 1e-3 bar


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


@pytest.mark.parametrize('agg', cases.AGGS)
def test_float64_restatement_reproduces_the_reference(golden, agg):
    slots, W1, b1, w2, b2, labels = cases.fixture_case(agg)
    ref = cases.forward64(slots, W1, b1, w2, b2, agg)
    logits = ref['logits'][0]
    assert rel_err(logits, golden[f'{agg}_logits']) < 1e-6
    assert abs(cases.loss64(logits, labels) - float(golden[f'{agg}_vqa_loss'])) < 1e-6 * abs(float(golden[f'{agg}_vqa_loss']))
    assert json.loads(str(golden[f'{agg}_acc_keys'])) == [f'acc_{t:.2f}' for t in cases.EVAL_THRESHS]
    acc = [cases.hits64(logits, labels, t).mean() for t in cases.EVAL_THRESHS]
    assert np.array_equal(np.float32(acc), golden[f'{agg}_acc'])
    # gradients at the float64 route (the fixture has no ties)
    t_star = ref['t_star'][0]
    B = len(labels)
    pair_star = np.stack([ref['rel'][0][b, t_star[b]].argmax(0) for b in range(B)])
    dW1, db1, dw2, db2 = cases.grads64(slots, W1[0], b1[0], w2[0], agg, cases.dloss64(logits, labels), t_star, pair_star)
    step = int(golden['dW1_row_step'])
    assert rel_err(dW1[::step], golden[f'{agg}_dW1_rows']) < 1e-6
    assert rel_err(db1, golden[f'{agg}_db1']) < 1e-6
    assert rel_err(dw2, golden[f'{agg}_dw2']) < 1e-6
    assert abs(db2 - float(golden[f'{agg}_db2'][0])) < 1e-6 * abs(db2)


def test_state_dict_contract(golden):
    from slotformer_amd.physion_vqa.models import PhysionReadout
    sd = PhysionReadout().state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == json.loads(str(golden['state_dict_keys']))
    assert sd['comb_idx'].tolist() == [i for p in cases.pairs_of(6) for i in p]
    cfg = json.loads(str(golden['config']))
    m = PhysionReadout(cfg['readout_dict'])
    assert (m.num_slots, m.slot_size, m.feats_dim, m.agg_func) == (6, 192, 192, 'max')
    assert m.dtype == torch.float32 and m.device.type == 'cpu'


class _Params:
    model = 'PhysionReadout'
    readout_dict = dict(num_slots=6, slot_size=192, agg_func='mean', feats_dim=192)


def test_build_model_through_both_packages():
    import slotformer_amd.physion_vqa as native
    alias = importlib.import_module('slotformer.physion_vqa')
    assert alias is native
    from slotformer.physion_vqa.models import PhysionReadout
    for pkg in (native, alias):
        m = pkg.build_model(_Params())
        assert isinstance(m, PhysionReadout) and m.agg_func == 'mean'
    nope = _Params()
    nope.model = 'PhyreReadout'
    with pytest.raises(NotImplementedError):
        native.build_model(nope)
    with pytest.raises(NotImplementedError):
        native.build_dataset(_Params())
    with pytest.raises(NotImplementedError):
        native.build_method()


def test_no_cpu_fallback_and_unsupported_shapes():
    from slotformer_amd.physion_vqa import evaluate, fit
    from slotformer_amd.physion_vqa.models import PhysionReadout
    from slotformer_amd import harness, ops
    m = PhysionReadout()
    slots = torch.zeros(2, 3, 6, 192)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m({'slots': slots})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_train_loss({'label': torch.zeros(2)}, {'logits': torch.zeros(2)})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_eval_loss({'label': torch.zeros(2)}, {'logits': torch.zeros(2)})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fit(m, slots, torch.zeros(2), 1, 2, 1e-3, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        evaluate(m, slots, torch.zeros(2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harness.readout_video_slots(m, slots, 2)
    # an unsupported readout_dict constructs and loads, and is refused with the limits at first use
    odd = PhysionReadout(dict(num_slots=17, slot_size=100, agg_func='max', feats_dim=48))
    odd.load_state_dict(odd.state_dict())
    with pytest.raises(NotImplementedError, match='multiples of 32'):
        odd({'slots': torch.zeros(1, 1, 17, 100)})
    assert ops.physion_readout_ok(6, 192, 192) and ops.physion_readout_ok(2, 32, 256) and ops.physion_readout_ok(16, 256, 32)
    for bad in ((1, 192, 192), (17, 192, 192), (6, 100, 192), (6, 288, 192), (6, 192, 48), (6, 192, 288), (6, 0, 192)):
        assert not ops.physion_readout_ok(*bad), bad


def test_abi_argument_errors():
    """Negative return codes with a message, before any HIP call."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)

    def err():
        return lib.sf_last_error_string().decode()

    def fwd(slots=one, N=6, Cc=192, F=192, T=5, agg=0, st=6 * 192):
        return lib.sf_physion_readout_fwd_f32(slots, 5 * st, st, 4, None, one, one, one, one, one, one, None, None, 1, 4, T, N, Cc, F, agg, None)

    def bwd(slots=one, N=6, Cc=192, F=192, T=5, agg=0, ws_bytes=1 << 30):
        return lib.sf_physion_readout_bwd_f32(slots, 5 * 6 * 192, 6 * 192, 4, None, one, one, one, one, one, None, one, one, one, one, 4, T, N, Cc, F,
                                              agg, one, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(slots=None) < 0 and 'null pointer' in err()
        for kw in (dict(N=1), dict(N=17), dict(Cc=100), dict(Cc=288), dict(F=48), dict(F=288)):
            assert call(**kw) < 0 and 'unsupported shape' in err() and 'multiples of 32' in err(), kw
        assert call(T=0) < 0 and 'T >= 1' in err()
        assert call(agg=3) < 0 and 'unknown aggregate' in err()
    assert fwd(st=6 * 192 - 4) < 0 and 'frame stride' in err()
    assert bwd(ws_bytes=16) < 0 and 'workspace too small' in err()
    assert lib.sf_physion_readout_bwd_workspace_bytes(4, 6, 192) == 4 * 192 * 13 * 4
    assert lib.sf_physion_readout_bwd_workspace_bytes(4, 17, 192) == 0
    th = (C.c_float * 17)(*([0.5] * 17))
    assert lib.sf_physion_readout_score_f32(None, one, None, th, 1, 0, None, None, None, None, 1, 4, None) < 0 and 'null pointer' in err()
    assert lib.sf_physion_readout_score_f32(one, one, None, th, 17, 0, None, None, None, None, 1, 4, None) < 0 and 'at most 16 thresholds' in err()
    assert lib.sf_physion_readout_score_f32(one, one, None, th, 1, 0, None, None, None, one, 1, 4, None) < 0 and 'per-task counts' in err()
    assert lib.sf_physion_readout_score_f32(one, one, None, th, 1, 0, None, None, None, None, 1, 0, None) < 0 and 'B >= 1' in err()
    assert lib.sf_physion_readout_ok(6, 192, 192) == 1 and lib.sf_physion_readout_ok(6, 192, 200) == 0


def test_batch_schedule_is_a_function_of_the_seed():
    from slotformer_amd.physion_vqa import batch_schedule
    a, b, c = batch_schedule(37, 3, 8, 5), batch_schedule(37, 3, 8, 5), batch_schedule(37, 3, 8, 6)
    flat = lambda s: [x.tolist() for e in s for x in e]
    assert flat(a) == flat(b) and flat(a) != flat(c)
    assert len(a) == 3 and [len(x) for x in a[0]] == [8, 8, 8, 8, 5]
    for epoch in a:
        assert sorted(int(i) for x in epoch for i in x) == list(range(37)) and all(x.dtype == torch.int32 for x in epoch)
    assert flat([a[0]]) != flat([a[1]])
    with pytest.raises(ValueError):
        batch_schedule(0, 1, 8, 5)


@pytest.mark.parametrize('shape', cases.FORWARD_CASES, ids=lambda s: '-'.join(map(str, s)))
def test_emulation_distance_of_the_gpu_cases(shape):
    d = cases.emulation_distance(cases.forward_case(shape), shape[-1])
    print(f'{shape}: emulated split-bf16 vs float64 = {d:.3e} of the largest |logit|')
    assert d < EMULATION_BOUND


def test_emulation_distance_of_the_fixture_and_the_other_gpu_inputs():
    for agg in cases.AGGS:
        d = cases.emulation_distance(cases.fixture_case(agg)[:5], agg)
        print(f'fixture {agg}: {d:.3e}')
        assert d < EMULATION_BOUND
    for args, agg in cases.OTHER_GPU_CASES:
        d = cases.emulation_distance(cases.seeded_case(*args), agg)
        print(f'{args} {agg}: {d:.3e}')
        assert d < EMULATION_BOUND
