"""CPU: CLEVRER VQA without a device -- the float64 restatement of tests/clevrer_vqa_cases.py against the REFERENCE's own results
(tests/golden/clevrer_aloe.npz, tools/gen_golden_clevrer_vqa.py), the model's state-dict contract, factory and the suffix remapping of a foreign
encoder layout, the refusals (training mode, CPU, mask_obj_loss, every limit of sf_aloe_ok one step inside and one step outside, the argument
errors of the C ABI, raised before any HIP call), the host assembly of the result records against the loop of test_clevrer_vqa.py, the
bookkeeping of calc_eval_loss restated in numpy, and the answer clearance of every seeded GPU case."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import clevrer_vqa_cases as cases

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# float64 restatement vs the reference's float32 forward over 12 layers, of the largest |logit|: measured 6.1e-7 (descriptive) and 4.7e-7
# (multiple choice; profiles/clevrer_vqa.md); ten times the larger
RESTATEMENT_BOUND = 6e-6


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN_DIR, 'clevrer_aloe.npz'))


@pytest.fixture(scope='module')
def fixture64():
    """the fixture's logits in float64, computed once: (fc, cls [3, 22], mc [3])"""
    fc = cases.fixture_case()
    cls = cases.forward64(fc['sd'], fc['cfg'], fc['slots'], fc['cls_tokens'], fc['cls_pad'], False)
    mc = cases.forward64(fc['sd'], fc['cfg'], fc['slots'], fc['mc_tokens'], fc['mc_pad'], True, video_index=fc['mc_video'][fc['mc_flag']])
    return fc, cls, mc


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def params_from_fixture(name='clevrer_vqa/configs/aloe_clevrer_params-rollout.py'):
    """a params file's settings as the BaseParams subclass the file defines; vocab_file points at the committed copy of the vocabulary"""
    with open(os.path.join(GOLDEN_DIR, 'clevrer_vqa_params.json')) as f:
        entry = json.load(f)['files'][name]
    names = {}
    for imp in entry['imports']:
        module, attr = imp.rsplit('.', 1)
        names[attr] = getattr(importlib.import_module(module), attr)
    attrs = dict(entry['attrs'], vocab_file=os.path.join(GOLDEN_DIR, 'clevrer_vocab.json'))
    assert entry['attrs']['vocab_file'] == 'CLEVRER_vocab.json'
    return type('SlotFormerParams', (names['BaseParams'], ), attrs)()


def test_float64_restatement_reproduces_the_reference(golden, fixture64):
    fc, cls, mc = fixture64
    cfg = json.loads(str(golden['config']))
    assert (cfg['transformer_dict'], cfg['lang_dict'], cfg['vision_dict'], cfg['loss_dict']) == tuple(fc['cfg'])
    for name, got in (('cls_logits', cls), ('mc_logits', mc)):
        d = rel_err(got, golden[name])
        print(f'float64 restatement vs the reference fixture, {name}: {d:.3e} of the largest |logit|')
        assert got.shape == golden[name].shape and d < RESTATEMENT_BOUND
    assert abs(cases.ce64(cls, fc['cls_label']) - float(golden['cls_answer_loss'])) < 2e-6 * float(golden['cls_answer_loss'])
    assert abs(cases.bce64(mc, fc['mc_label']) - float(golden['mc_answer_loss'])) < 2e-6 * float(golden['mc_answer_loss'])
    assert list(golden['train_bs']) == [3, 3]
    # calc_eval_loss: the reference's keys in its order, its values from the restated bookkeeping
    want, _ = cases.eval_reference(cls, fc['cls_label'], mc, fc['mc_label'], fc['mc_flag'], fc['mc_subtype'])
    assert json.loads(str(golden['eval_keys'])) == list(want)
    assert np.allclose(golden['eval_values'], [float(v) for v in want.values()], rtol=0, atol=1e-7)
    assert want['descriptive_acc'] == pytest.approx(2 / 3) and want['multiple-choice_acc'] == 0.5 and want['explanatory_bs'] == 1   # (not all zero)
    # the padding is dead in the restatement too: other tokens at padded places, the same logits
    tokens = fc['cls_tokens'].copy()
    tokens[fc['cls_pad']] = 5
    assert np.array_equal(cases.forward64(fc['sd'], fc['cfg'], fc['slots'][:1], tokens[:1], fc['cls_pad'][:1], False), cls[:1])


def test_every_seeded_case_clears_the_answer_bar(fixture64):
    """No case left out: descriptive top-2 gap > 2 DEVICE_BAR max|logit|, multiple-choice |logit| > DEVICE_BAR max|logit| -- so a device within
    the bar gives exactly the float64 answers."""
    fc, cls, mc = fixture64
    rows = [('fixture-cls', cls, False), ('fixture-mc', mc, True)]
    rows += [(c['name'], cases.reference64(cases.forward_case(c)), bool(c.get('mc'))) for c in cases.FORWARD_CASES]
    h_cls, h_mc = cases.harness64(cases.harness_case())
    rows += [('harness-cls', h_cls, False), ('harness-mc', h_mc, True)]
    for name, logits, is_mc in rows:
        margin, bar = cases.clearance(logits, is_mc)
        print(f'{name}: margin {margin:.3e}, bar {bar:.3e}')
        assert margin > bar, name


def test_state_dict_contract_and_factory(golden):
    import slotformer_amd.clevrer_vqa as native
    alias = importlib.import_module('slotformer.clevrer_vqa')
    assert alias is native
    from slotformer.clevrer_vqa.models import CLEVRERAloe, CLEVRERTransformerModel
    want = json.loads(str(golden['state_dict_keys']))
    for name in ('clevrer_vqa/configs/aloe_clevrer_params-rollout.py', 'clevrer_vqa/configs/aloe_clevrer_params.py'):
        m = alias.build_model(params_from_fixture(name))
        assert isinstance(m, CLEVRERAloe) and isinstance(m.transformer_model, CLEVRERTransformerModel)
        tm = m.transformer_model
        assert (tm.d_model, tm.input_len, tm.question_len, tm.num_answer_classes, tm.q_embedding.num_embeddings) == (144, 208, 20, 22, 82)
        sd = m.state_dict()
        owned = [[k, list(v.shape)] for k, v in sd.items() if not k.startswith('transformer_model.transformer_encoder.')]
        assert owned == want                                     # the reference-owned parameters: keys, ORDER and shapes
        assert want == [['transformer_model.' + k, list(s)] for k, s in cases.owned_shapes(cases.config())]
        assert [[k, list(v.shape)] for k, v in sd.items()] == [['transformer_model.' + k, list(s)] for k, s in cases.state_shapes(cases.config())]
        assert m.dtype == torch.float32 and m.device.type == 'cpu' and tm.shape_ok(7, 25, 32)
        assert not any(p.requires_grad for p in (tm.text_token, tm.vision_token, tm.cls_token, tm.mc_question_token, tm.mc_choice_token))
        assert tm.CLS.abs().max() == 0
    m.load_state_dict({'transformer_model.' + k: v for k, v in cases.seeded_weights(cases.config(), 1).items()})   # strict
    nope = params_from_fixture()
    nope.model = 'CLEVRERAloeV2'
    with pytest.raises(NotImplementedError):
        native.build_model(nope)
    with pytest.raises(NotImplementedError):
        native.build_dataset(nope)
    with pytest.raises(NotImplementedError):
        native.build_method()


@pytest.mark.parametrize('between', ['encoder.', 'model.tfm.blocks.'])
def test_foreign_encoder_layout_loads_by_suffix(between):
    """Two made-up wrapper layouts: whatever stands between the encoder's prefix and `layers.i.<leaf>`, and whatever the position table is
    called, the tensors land in layer i and in pos_enc."""
    from slotformer_amd.clevrer_vqa.models import CLEVRERAloe, CLEVRERTransformerModel
    cfg = cases.config(T=2, N=3, C=32, text_len=5, heads=2, nl=3, ffn=64)
    sd = cases.seeded_weights(cfg, 3)
    pre = 'transformer_encoder.'
    foreign = {}
    for k, v in sd.items():
        if k == pre + 'pos_enc':
            foreign[pre + ('pe.table' if between == 'encoder.' else 'position_embedding')] = v[0] if between == 'encoder.' else v
        elif k.startswith(pre):
            foreign[pre + between + k[len(pre):]] = v
        else:
            foreign[k] = v
    tm = CLEVRERTransformerModel(*cfg)
    tm.load_state_dict(foreign)
    for k, v in tm.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m = CLEVRERAloe(CLEVRERTransformerModel(*cfg))
    m.load_state_dict({'transformer_model.' + k: v for k, v in foreign.items()})
    for k, v in m.transformer_model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # anything else under the prefix is an error that names the keys; so are two candidate tables
    extra = dict(foreign, **{pre + between + 'final_norm.weight': torch.zeros(36)})
    with pytest.raises(KeyError, match='final_norm.weight'):
        tm.load_state_dict(extra)
    two = dict(foreign, **{pre + 'another_table': sd[pre + 'pos_enc'][0].clone()})
    with pytest.raises(KeyError, match='another_table'):
        tm.load_state_dict(two)


def test_refusals_training_cpu_mask_obj_loss():
    from slotformer_amd import harness, ops
    from slotformer_amd.clevrer_vqa.models import CLEVRERAloe, CLEVRERTransformerModel
    cfg = cases.config(T=2, N=3, C=32, text_len=5, heads=2, nl=1, ffn=64)
    m = CLEVRERAloe(CLEVRERTransformerModel(*cfg))
    data = {'cls_video_emb': torch.zeros(2, 2, 3, 32), 'cls_q_tokens': torch.zeros(2, 5, dtype=torch.long), 'cls_q_pad_mask': torch.zeros(2, 5, dtype=torch.bool),
            'mc_q_tokens': torch.zeros(0, 5, dtype=torch.long), 'mc_q_pad_mask': torch.zeros(0, 5, dtype=torch.bool), 'mc_flag': torch.zeros(0, dtype=torch.long)}
    assert m.training
    with pytest.raises(NotImplementedError, match='backward of the Aloe reasoner .* not built'):
        m(data)
    m.eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(data)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_train_loss({'cls_label': torch.zeros(2)}, {'cls_answer_logits': torch.zeros(2, 22), 'mc_answer_logits': None})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.calc_eval_loss({'cls_label': torch.zeros(2)}, {'cls_answer_logits': torch.zeros(2, 22), 'mc_answer_logits': None})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        harness.clevrer_answers(m, torch.zeros(2, 2, 3, 32), {})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.aloe_score(torch.zeros(2, 3), torch.zeros(2))
    with pytest.raises(AssertionError, match='mask_obj_loss'):
        CLEVRERTransformerModel(cfg[0], cfg[1], cfg[2], dict(use_mask_obj_loss=True))
    with pytest.raises(NotImplementedError, match='learnable'):
        CLEVRERTransformerModel(dict(cfg[0], pos_enc='sin'), cfg[1], cfg[2], cfg[3])


def test_limits_one_step_inside_and_outside():
    """sf_aloe_ok(N, C, T, text_len, d_model, heads, ffn, layers): every limit, one step inside and one step outside."""
    from slotformer_amd import ops
    ok = ops.aloe_ok
    assert ok(7, 128, 25, 32, 144, 8, 512, 12)                                           # the reference shape
    assert ok(1, 128, 25, 32, 144, 8, 512, 12) and not ok(0, 128, 25, 32, 144, 8, 512, 12)        # slots 1 | 0
    assert ok(16, 128, 2, 32, 144, 8, 512, 12) and not ok(17, 128, 2, 32, 144, 8, 512, 12)       # slots 16 | 17
    assert ok(7, 32, 25, 32, 144, 8, 512, 12) and not ok(7, 0, 25, 32, 144, 8, 512, 12)          # C 32 | 0
    assert ok(7, 256, 25, 32, 144, 8, 512, 12) and not ok(7, 288, 25, 32, 144, 8, 512, 12)       # C 256 | 288
    assert not ok(7, 100, 25, 32, 144, 8, 512, 12) and not ok(7, 130, 25, 32, 144, 8, 512, 12)   # C no multiple of 32
    assert ok(7, 128, 1, 32, 144, 8, 512, 12) and not ok(7, 128, 0, 32, 144, 8, 512, 12)         # frames 1 | 0
    assert ok(7, 128, 25, 1, 144, 8, 512, 12) and not ok(7, 128, 25, 0, 144, 8, 512, 12)         # text 1 | 0
    assert ok(7, 128, 25, 80, 144, 8, 512, 12) and not ok(7, 128, 25, 81, 144, 8, 512, 12)       # 256 | 257 tokens
    assert ok(15, 128, 16, 15, 144, 8, 512, 12) and not ok(16, 128, 16, 1, 144, 8, 512, 12)      # 256 | 258 tokens
    assert ok(7, 128, 25, 32, 32, 8, 512, 12) and not ok(7, 128, 25, 32, 16, 8, 512, 12)         # head dim 4 | 2
    assert ok(7, 128, 25, 32, 256, 8, 512, 12) and not ok(7, 128, 25, 32, 272, 8, 512, 12)       # head dim 32 | 34
    assert ok(7, 128, 25, 32, 144, 8, 512, 12) and not ok(7, 128, 25, 32, 136, 8, 512, 12)       # head dim 18 | 17 (odd)
    assert ok(7, 128, 25, 32, 256, 16, 512, 12) and not ok(7, 128, 25, 32, 288, 16, 512, 12)     # d_model 256 | 288
    assert not ok(7, 128, 25, 32, 144, 7, 512, 12) and not ok(7, 128, 25, 32, 144, 0, 512, 12)   # d_model no multiple of heads; no head
    assert ok(7, 128, 25, 32, 12, 2, 512, 12) and not ok(7, 128, 25, 32, 6, 1, 512, 12)          # d_model a multiple of 4 (the GEMM's K): 12 | 6
    assert ok(7, 128, 25, 32, 144, 8, 64, 12) and not ok(7, 128, 25, 32, 144, 8, 0, 12)          # ffn 64 | 0
    assert ok(7, 128, 25, 32, 144, 8, 1024, 12) and not ok(7, 128, 25, 32, 144, 8, 1088, 12)     # ffn 1024 | 1088
    assert not ok(7, 128, 25, 32, 144, 8, 500, 12)                                               # ffn no multiple of 64
    assert ok(7, 128, 25, 32, 144, 8, 512, 1) and not ok(7, 128, 25, 32, 144, 8, 512, 0)         # layers 1 | 0
    assert ok(7, 128, 25, 32, 144, 8, 512, 32) and not ok(7, 128, 25, 32, 144, 8, 512, 33)       # layers 32 | 33
    # the class's default head count (10 heads of 18) is covered; post-LN is not, whatever the shape
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel
    cfg = cases.config(T=2, N=3, C=32, text_len=5, heads=10, nl=1, ffn=64)
    assert CLEVRERTransformerModel(*cfg).shape_ok(3, 2, 5)
    assert not CLEVRERTransformerModel(dict(cfg[0], norm_first=False), *cfg[1:]).shape_ok(3, 2, 5)


def test_abi_argument_errors():
    """Negative return codes with a message, before any HIP call."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.sf_last_error_string().decode()  # noqa: E731
    one = C.c_void_p(16)
    layers = (_lib.sf_tfm_layer * 1)()
    m = _lib.sf_aloe()
    m.num_slots, m.slot_size, m.T, m.text_len, m.question_len = 3, 32, 2, 5, 5
    m.d_model, m.num_heads, m.ffn_dim, m.num_layers, m.vocab, m.emb_dim = 36, 2, 64, 1, 10, 14
    for name in ('cls', 'pos', 'vision_w', 'vision_b', 'q_in_proj_w', 'text_table'):
        setattr(m, name, 16)
    m.layers = C.cast(layers, C.POINTER(_lib.sf_tfm_layer))

    def fwd(model=m, slots=one, stride_t=96, V=4, vidx=None, hidden=8, outputs=3, B=2, ws=1 << 30):
        return lib.sf_aloe_fwd_f32(C.byref(model), slots, 192, stride_t, V, 2, vidx, None, 1, one, one, 0, one, one, one, one, hidden, outputs, one, None,
                                   B, one, ws, None)

    assert fwd(slots=None) < 0 and 'null pointer' in err()
    bad = _lib.sf_aloe.from_buffer_copy(m)
    bad.slot_size = 100
    assert fwd(model=bad) < 0 and 'multiple of 32' in err()
    bad = _lib.sf_aloe.from_buffer_copy(m)
    bad.text_len = 250
    assert fwd(model=bad) < 0 and '<= 256' in err()
    bad = _lib.sf_aloe.from_buffer_copy(m)
    bad.vocab = 0
    assert fwd(model=bad) < 0 and 'vocab' in err()
    assert fwd(stride_t=95) < 0 and 'stride' in err()
    assert fwd(B=5) < 0 and 'video_index' in err()
    assert fwd(B=0) < 0 and fwd(B=70000) < 0 and 'B <= 65535' in err()
    assert fwd(hidden=2000) < 0 and fwd(outputs=0) < 0 and 'mlp_hidden' in err()
    assert fwd(slots=C.c_void_p(20)) < 0 and '16-byte aligned' in err()
    assert fwd(ws=1024) < 0 and 'workspace too small' in err()
    assert fwd() < 0 and 'null pointer in a layer' in err()          # everything else passes: the first layer's pointers are checked last
    old = lib.sf_get_precision()
    try:
        for mode in (0, 2):
            lib.sf_set_precision(mode)
            assert fwd() < 0 and 'split-bf16' in err()
    finally:
        lib.sf_set_precision(old)
    assert lib.sf_aloe_workspace_bytes(2, 3, 2, 5, 36, 64) == 2 * 12 * (6 * 36 + 64) * 4
    assert lib.sf_aloe_workspace_bytes(0, 3, 2, 5, 36, 64) == 0 and lib.sf_aloe_workspace_bytes(2, 17, 2, 5, 36, 64) == 0
    assert lib.sf_aloe_text_table_f32(None, one, one, one, 10, 14, 36, None) < 0 and 'null pointer' in err()
    assert lib.sf_aloe_text_table_f32(one, one, one, one, 0, 14, 36, None) < 0 and 'vocab' in err()
    assert lib.sf_aloe_score_f32(None, None, 2, 3, None, None, None, 0, None, 0, None, None, None, None) < 0 and 'descriptive' in err()
    assert lib.sf_aloe_score_f32(None, None, 0, 0, one, None, None, 2, None, 0, None, None, None, None) < 0 and 'multiple-choice' in err()
    assert lib.sf_aloe_score_f32(None, None, 0, 0, None, None, None, 0, None, 2, None, None, None, None) < 0 and 'ques_correct' in err()


def test_result_records_against_the_reference_loop():
    """clevrer_vqa.result_records on the answers of two batches against the loop of test_clevrer_vqa.py restated in numpy: descriptive questions,
    multiple-choice questions with 4, 4, 3, 1 choices, a question whose choices are split over two batches (its entry is extended)."""
    from slotformer_amd import clevrer_vqa
    rng = np.random.default_rng(5)
    label2answer = {i: f'word{i}' for i in range(22)}
    batches, cls_all, mc_all, q = [], [], [], dict(cls_scene_index=[], cls_question_id=[], mc_scene_index=[], mc_question_id=[], mc_flag=[], mc_choice_id=[])
    n_q = 0
    # (batch 1 reuses question id 4 of scene 15007: its choices are appended to the entry batch 0 made)
    for choices, n_cls, scenes, ids in (([4, 4, 3, 1], 3, [15000, 15007, 19999], [0, 1, 2, 3, 4, 5, 6]), ([2, 3], 2, [15007, 15003], [10, 11, 4, 12])):
        n_mc = len(choices)
        scene = np.array([scenes[i % len(scenes)] for i in range(n_cls + n_mc)], np.int32)
        qid = np.array(ids, np.int32)
        flag = np.repeat(np.arange(n_mc), choices)
        cid = np.concatenate([np.arange(c) for c in choices])
        cls_ans, mc_ans = rng.integers(0, 22, n_cls), rng.uniform(size=len(flag)) > 0.5
        batches.append(dict(scene_index=scene, question_id=qid, mc_choice_id=cid, mc_flag=flag, cls_answer=cls_ans, mc_answer=mc_ans))
        cls_all.append(cls_ans)
        mc_all.append(mc_ans)
        q['cls_scene_index'] += list(scene[:n_cls])
        q['cls_question_id'] += list(qid[:n_cls])
        q['mc_scene_index'] += list(scene[n_cls:])
        q['mc_question_id'] += list(qid[n_cls:])
        q['mc_flag'] += list(flag + n_q)
        q['mc_choice_id'] += list(cid)
        n_q += n_mc
    want = cases.records_reference(batches, label2answer)
    # the reference walks batch by batch (descriptive, then multiple choice, per batch); the harness returns all descriptive answers, then all
    # choices -- the records of a scene hold the same entries, the order inside a scene's list follows the walk
    got = clevrer_vqa.result_records(np.concatenate(cls_all), np.concatenate(mc_all), q, label2answer)
    assert len(got) == 5000 and [r['scene_index'] for r in got] == [r['scene_index'] for r in want]
    key = lambda e: (e['question_id'], 'choices' in e)  # noqa: E731
    for g, w in zip(got, want):
        assert sorted(g['questions'], key=key) == sorted(w['questions'], key=key), g['scene_index']
    assert sum(len(r['questions']) for r in got) == 5 + 6 - 1
    # one batch alone: the same order too
    b0 = batches[0]
    q0 = dict(cls_scene_index=b0['scene_index'][:3], cls_question_id=b0['question_id'][:3], mc_scene_index=b0['scene_index'][3:],
              mc_question_id=b0['question_id'][3:], mc_flag=b0['mc_flag'], mc_choice_id=b0['mc_choice_id'])
    assert clevrer_vqa.result_records(b0['cls_answer'], b0['mc_answer'], q0, label2answer) == cases.records_reference([b0], label2answer)


def test_eval_bookkeeping_restatement():
    """The numpy restatement itself, on runs of 4, 4, 3, 1 choices with a known outcome, and with empty kinds."""
    flag = np.repeat(np.arange(4), [4, 4, 3, 1])
    labels = np.array([1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1], np.float32)
    logits = np.where(labels > 0, 2.0, -2.0)
    logits[5] = 0.7                       # question 1 gets one choice wrong
    logits[11] = 0.0                      # logit 0 is 'wrong': question 3 (label 1) fails
    got, corr = cases.eval_reference(None, None, logits, labels, flag, np.array([1, 2, 3, 3]))
    assert list(corr) == [True, False, True, False]
    assert got == {'descriptive_acc': 0., 'descriptive_bs': 0, 'multiple-choice_acc': 0.5, 'multiple-choice_bs': 4, 'explanatory_acc': 1.0,
                   'explanatory_bs': 1, 'predictive_acc': 0.0, 'predictive_bs': 1, 'counterfactual_acc': 0.5, 'counterfactual_bs': 2}
    got, corr = cases.eval_reference(np.eye(3), [0, 1, 0], None, None, None, np.zeros(0))
    assert corr is None and got['descriptive_acc'] == pytest.approx(2 / 3) and got['multiple-choice_bs'] == 0 and got['counterfactual_bs'] == 0
