"""CPU: the training path of the Aloe reasoner without a device -- the float64 restatement of tests/aloe_fit_cases.py against the REFERENCE's
gradients (tests/golden/clevrer_aloe_grads.npz, tools/gen_golden_clevrer_vqa_grads.py), the ABI of the new calls and every refusal on both sides of
its limit with no HIP call, the gradient layout against the parameters, the host-side validation of `fit`, the question schedule, and the float64
run of the planted set that fixes the epoch count of the GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import aloe_fit_cases as fc
import clevrer_vqa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_the_reference_gradients():
    ref = fc.loss_and_grads64(fc.fixture_train_case())
    worst = fc.check_against_golden(ref['grads'], ref['losses'], 1e-5)   # (the file holds the reference's float32 results)
    print(f'float64 restatement vs the reference fixture: worst relative error {worst:.2e}')
    g = np.load(fc.GOLDEN)
    assert fc.rel_err(ref['cls_logits'], g['cls_logits']) < 1e-5 and fc.rel_err(ref['mc_logits'], g['mc_logits']) < 1e-5
    assert os.path.getsize(fc.GOLDEN) < 900_000
    assert all(np.abs(g['grad.' + k]).max() > 0 for k in fc.grad_keys(fc.fixture_train_case()['cfg']))   # every leaf is reached


def test_cases_cover_the_table_of_the_issue():
    by = {c['name']: c for c in fc.CASES}
    L = lambda c: 1 + c['T'] * c['N'] + c['text_len']  # noqa: E731
    live = lambda c: [1 + c['T'] * c['N'] + n for n in c['cls_lengths']] + [  # noqa: E731
        1 + c['T'] * c['N'] + min(n, c['ql']) + k for n, k in zip(c['mc_lengths'], c['choice_lengths'])]
    rows = lambda c: (len(c['cls_lengths']) + len(c['mc_lengths'])) * L(c)  # noqa: E731
    t = by['tiny-L6']
    assert (L(t), t['T'], t['N'], t['text_len'], t['nl'], t['ffn']) == (6, 1, 1, 4, 1, 64)
    assert live(by['live-15-16-17-b1-only']) == [15, 16, 17] and not by['live-15-16-17-b1-only']['mc_lengths']
    assert live(by['live-31-32-33-bn-only']) == [31, 32, 33] and not by['live-31-32-33-bn-only']['cls_lengths']
    assert L(by['L256-full']) == 256 and live(by['L256-full'])[0] == 256
    r = by['reference-geometry']
    assert (L(r), r['input_dim'] + 2, r['nl'], len(live(r))) == (208, 18, 2, 3)
    assert by['hd6']['input_dim'] + 2 == 6 and by['hd32']['input_dim'] + 2 == 32
    m = by['mc-padding-inside-one-choice']
    assert m['mc_flag'] == [0, 0, 1] and any(n < m['ql'] for n in m['mc_lengths']) and any(m['ql'] + k < m['text_len'] for k in m['choice_lengths'])
    assert {c['p'] for c in fc.CASES} == {0.0, 0.1}
    s = by['strided-nan-start-offset']
    assert s['strided'] and s['frame_offset'] == 2 and max(s['start']) + (s['T'] - 1) * 2 < s['T_all']
    v = by['video-index-shuffled']
    assert sorted(v['video_index']) != v['video_index'] and len(set(v['video_index'])) < len(v['video_index'])
    assert any(rows(c) % 32 for c in fc.CASES)
    assert rows(by['rows64']) == 64 and rows(by['rows65']) == 65
    assert (by['n16-c256']['N'], by['n16-c256']['C']) == (16, 256)
    assert all(c['nl'] <= 2 and len(live(c)) <= 5 for c in fc.CASES)


def header_text():
    txt = open(os.path.join(ROOT, 'include', 'slotformer_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


NEW_CALLS = ('sf_aloe_train_ok', 'sf_aloe_train_workspace_bytes', 'sf_aloe_train_fwd_f32', 'sf_aloe_train_bwd_f32', 'sf_aloe_score_grad_f32')


def test_symbols_are_declared_exported_and_mirrored():
    from slotformer_amd import _lib, build
    lib = _lib.lib()
    txt = header_text()
    for name in NEW_CALLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = txt[txt.index(name + '('):]
        assert decl[:decl.index(';')].count(',') + 1 == len(_lib.SIGNATURES[name][1]), name
    assert 'aloe_train.hip' in build.SOURCES

    def fields(name):
        end = txt.index('} ' + name + ';')
        body = txt[txt.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
        out = []
        for decl in body.split(';'):
            decl = re.sub(r'^(const\s+)?(float|int|sf_tfm_layer_grads|sf_tfm_layer)\s*', '', decl.strip())
            out += [re.sub(r'[\*\s]', '', f) for f in decl.split(',') if f.strip()]
        return out

    assert [f[0] for f in _lib.sf_aloe_model._fields_] == fields('sf_aloe_model')
    assert [f[0] for f in _lib.sf_aloe_grads._fields_] == fields('sf_aloe_grads')
    assert C.sizeof(_lib.sf_aloe_model) == 13 * 4 + 4 + 16 * 8 and C.sizeof(_lib.sf_aloe_grads) == 16 * 8


def dummy_model(N=7, Cs=128, T=25, TL=32, d=144, heads=8, ffn=512, nl=12, H=128, A=22, vocab=82, E=14, ptr=4096):
    """a descriptor whose device pointers are a non-null, aligned dummy: every case below is refused before one is dereferenced"""
    from slotformer_amd import _lib
    m = _lib.sf_aloe_model()
    m.num_slots, m.slot_size, m.T, m.text_len, m.question_len, m.d_model, m.num_heads, m.ffn_dim, m.num_layers = N, Cs, T, TL, 20, d, heads, ffn, nl
    m.vocab, m.emb_dim, m.mlp_hidden, m.num_answers = vocab, E, H, A
    g = _lib.sf_aloe_grads()
    for f in _lib._ALOE_LEAVES + _lib._ALOE_HEADS:
        setattr(m, f, ptr)
        setattr(g, f, ptr)
    arr, garr = (_lib.sf_tfm_layer * max(nl, 1))(), (_lib.sf_tfm_layer_grads * max(nl, 1))()
    for layer, glayer in zip(arr, garr):
        for f, _ in _lib.sf_tfm_layer_grads._fields_:
            setattr(layer, f, ptr)
            setattr(glayer, f, ptr)
    m.layers, g.layers = C.cast(arr, C.POINTER(_lib.sf_tfm_layer)), C.cast(garr, C.POINTER(_lib.sf_tfm_layer_grads))
    return m, g, (arr, garr)


def test_shape_limits_on_both_sides():
    from slotformer_amd import _lib, ops
    lib = _lib.lib()
    ok = lambda **kw: ops.aloe_train_ok(*[{**dict(N=7, C=128, T=25, TL=32, d=144, heads=8, ffn=512, nl=12), **kw}[k]  # noqa: E731
                                           for k in ('N', 'C', 'T', 'TL', 'd', 'heads', 'ffn', 'nl')])
    assert ok()                                                     # the reference shape
    assert ok(N=16, T=13, TL=47) and not ok(N=17, T=1)              # slots
    assert ok(C=32) and ok(C=256) and not ok(C=288) and not ok(C=48) and not ok(C=0)
    assert ok(T=31, TL=38) and not ok(T=31, TL=39)                  # 256 tokens and 257
    assert not ok(T=0) and not ok(TL=0)
    assert ok(d=256, heads=8) and not ok(d=264, heads=12)           # d_model
    assert ok(d=32, heads=8) and not ok(d=16, heads=8)              # head dim 4 and 2
    assert ok(d=256, heads=8) and not ok(d=272, heads=8)            # head dim 32 and 34
    assert not ok(d=40, heads=8)                                    # an odd head dim
    assert ok(ffn=64) and ok(ffn=1024) and not ok(ffn=1088) and not ok(ffn=96) and not ok(ffn=0)
    assert ok(nl=1) and ok(nl=32) and not ok(nl=33) and not ok(nl=0)
    # everything sf_aloe_ok accepts, sf_aloe_train_ok accepts
    for c in cases.FORWARD_CASES:
        d = (c['input_dim'] + 2) * c['heads']
        assert ops.aloe_train_ok(c['N'], c['C'], c['T'], c['text_len'], d, c['heads'], c['ffn'], c['nl']) == \
            ops.aloe_ok(c['N'], c['C'], c['T'], c['text_len'], d, c['heads'], c['ffn'], c['nl'])
    q = lib.sf_aloe_train_workspace_bytes
    m = dummy_model()[0]
    assert q(C.byref(m), 1) > 0 and q(C.byref(m), 65535) > q(C.byref(m), 256) > q(C.byref(m), 64) and q(C.byref(m), 0) == 0 and q(C.byref(m), 65536) == 0
    assert q(None, 4) == 0
    for odd in (dict(N=17), dict(Cs=100), dict(nl=33), dict(nl=0), dict(H=0), dict(H=1025), dict(A=0), dict(A=1025), dict(vocab=0), dict(E=0)):
        assert q(C.byref(dummy_model(**odd)[0]), 4) == 0, odd
    for fine in (dict(H=1), dict(H=1024), dict(A=1), dict(A=1024), dict(vocab=1), dict(E=1)):
        assert q(C.byref(dummy_model(**fine)[0]), 4) > 0, fine


def test_argument_errors_without_a_gpu():
    from slotformer_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.sf_last_error_string().decode()  # noqa: E731
    one = C.c_void_p(4096)
    m, g, keep = dummy_model(nl=2)
    q = lib.sf_aloe_train_workspace_bytes
    big = 1 << 50

    def fwd(model=m, slots=one, sv=25 * 7 * 128, st=7 * 128, V=4, T_all=25, vi=None, tokens=one, pad=one, B1=2, Bn=1, p=0.1, cl=one, ml=one, ws=one,
            nbytes=big):
        return lib.sf_aloe_train_fwd_f32(C.byref(model) if model is not None else None, slots, sv, st, V, T_all, vi, None, 1, tokens, pad, B1, Bn, p, 7, cl,
                                         ml, None, None, ws, nbytes, None)

    def bwd(model=m, slots=one, sv=25 * 7 * 128, st=7 * 128, V=4, T_all=25, vi=None, tokens=one, pad=one, B1=2, Bn=1, p=0.1, cl=one, ml=one, grads=g,
            ws=one, nbytes=big):
        return lib.sf_aloe_train_bwd_f32(C.byref(model) if model is not None else None, slots, sv, st, V, T_all, vi, None, 1, tokens, pad, B1, Bn, cl, ml,
                                         C.byref(grads) if grads is not None else None, p, 7, ws, nbytes, None)

    old = lib.sf_get_precision()
    try:
        lib.sf_set_precision(1)
        for call in (fwd, bwd):
            assert call(model=None) < 0 and 'null pointer' in err()
            for name in ('slots', 'tokens', 'pad', 'ws'):
                assert call(**{name: None}) < 0 and 'null pointer' in err(), name
            assert call(cl=None) < 0 and 'null pointer' in err()
            assert call(ml=None) < 0 and 'null pointer' in err()
            for odd in (dict(Cs=100), dict(N=17), dict(T=32), dict(d=148), dict(ffn=96), dict(nl=33), dict(H=1025), dict(A=0), dict(vocab=0)):
                assert call(model=dummy_model(**odd)[0]) < 0 and 'unsupported shape' in err(), odd
            bad = dummy_model(nl=2)[0]
            bad.q_embedding = None
            assert call(model=bad) < 0 and 'null pointer in the model' in err()
            bad = dummy_model(nl=2)
            bad[0].layers[1].lin2_b = None
            assert call(model=bad[0]) < 0 and 'null pointer in a layer' in err()
            assert call(B1=-1) < 0 and 'B1 >= 0' in err()
            assert call(B1=0, Bn=0) < 0 and '1 <= B1 + Bn <= 65535' in err()
            assert call(B1=65535, Bn=1) < 0 and '1 <= B1 + Bn <= 65535' in err()
            assert call(B1=21000, Bn=0, vi=one) < 0 and 'batch too large' in err()          # 21000 x 208 x 512 >= 2^31
            assert call(V=0) < 0 and 'V >= 1' in err()
            assert call(B1=4, Bn=1) < 0 and 'video_index' in err()                           # 5 sequences, 4 videos, no index
            assert call(st=7 * 128 - 4) < 0 and 'stride' in err()
            assert call(sv=25 * 7 * 128 + 2) < 0 and 'stride' in err()
            assert call(p=1.0) < 0 and 'dropout_p' in err()
            assert call(p=-0.1) < 0 and 'dropout_p' in err()
            assert call(slots=C.c_void_p(4100)) < 0 and '16-byte aligned' in err()
            assert call(ws=C.c_void_p(4104)) < 0 and '16-byte aligned' in err()
            assert call(model=dummy_model(nl=2, ptr=4100)[0]) < 0 and '16-byte aligned' in err()
            assert call(nbytes=q(C.byref(m), 3) - 1) < 0 and 'workspace too small' in err()
            lib.sf_set_precision(0)
            assert call() < 0 and 'split-bf16' in err()
            lib.sf_set_precision(2)
            assert call() < 0 and 'split-bf16' in err()
            lib.sf_set_precision(1)
        assert bwd(grads=None) < 0 and 'null pointer' in err()
        bad = dummy_model(nl=2)[1]
        bad.pos = None
        assert bwd(grads=bad) < 0 and 'null pointer in the gradients' in err()
        odd_g = dummy_model(nl=2)[1]
        odd_g.layers[1].lin1_b = 4100
        assert bwd(grads=odd_g) < 0 and '16-byte aligned' in err()
        sg = lib.sf_aloe_score_grad_f32
        assert sg(one, one, -1, 9, one, one, 2, 1., 1., one, one, one, None) < 0 and 'B1 >= 0' in err()
        assert sg(None, one, 2, 9, one, one, 2, 1., 1., one, one, one, None) < 0 and 'descriptive' in err()
        assert sg(one, one, 2, 0, one, one, 2, 1., 1., one, one, one, None) < 0 and 'num_answers' in err()
        assert sg(one, one, 2, 9, one, None, 2, 1., 1., one, one, one, None) < 0 and 'multiple-choice' in err()
    finally:
        lib.sf_set_precision(old)
    del keep


def test_grad_layout_follows_the_parameters():
    from slotformer_amd import ops, train
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel
    for case in (fc.CASES[0], fc.CASES[4], fc.CASES[5]):
        cfg = fc.train_case(case)['cfg']
        tm = CLEVRERTransformerModel(*[dict(c) for c in cfg])
        m = cases.dims(cfg)
        params = train.aloe_parameters(tm)
        layout = ops.aloe_grad_layout(m['C'], m['L'], m['d'], m['ffn'], m['nl'], m['q_vocab'], m['E'], m['mlp'], m['a_vocab'])
        assert [k for _, k in layout] == [p.numel() for p in params]
        names = dict(tm.named_parameters())
        assert [names[k] is p for k, p in zip(fc.grad_keys(cfg), params)] == [True] * len(params)
        assert {id(p) for p in params} == {id(p) for p in tm.parameters() if p.requires_grad}          # every trainable leaf, once
        off = 0
        for (name, k), p in zip(layout, params):   # every leaf up to the layers' last starts on a multiple of four floats
            if not name.startswith(('cls_w', 'cls_b', 'mc_', 'q_embedding')):
                assert off % 4 == 0, name
            off += k
        tail = [n for n, _ in layout[-5:]]
        assert tail == ['q_embedding', 'cls_w2', 'cls_b2', 'mc_w2', 'mc_b2']   # the leaves of odd size come last


def test_cached_descriptor_survives_copies_and_is_dropped_with_the_plans(monkeypatch):
    """The autograd node keeps its ctypes descriptor in the module's plan cache: a module that went through it still deep-copies and pickles
    (the copies start without a descriptor), the descriptor is rebuilt when the geometry or a parameter's storage changes, and
    `plans.invalidate` -- which `fit` calls -- drops it."""
    import copy
    import pickle
    from slotformer_amd import plans, train
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel, CLEVRERAloe
    tm = CLEVRERTransformerModel(*[dict(c) for c in fc.train_case(fc.CASES[0])['cfg']])
    model = CLEVRERAloe(tm)
    built = []

    def fake(tm_, N, T, TL):   # (the real one wants device pointers; what matters here is what it returns: ctypes objects that hold pointers)
        m, _, keep = dummy_model(N=N, T=T, TL=TL, nl=1)
        built.append((N, T, TL))
        return m, [keep]

    monkeypatch.setattr(train, 'aloe_model', fake)
    a = train._aloe_model_cached(tm, 1, 1, 4)
    assert train._aloe_model_cached(tm, 1, 1, 4) is a and built == [(1, 1, 4)]
    with pytest.raises(ValueError, match='pointers'):
        pickle.dumps(a[0])                                   # the thing itself cannot be pickled ...
    for owner in (tm, model):                                # ... the modules that hold it can be copied and pickled all the same
        twin = copy.deepcopy(owner)
        back = pickle.loads(pickle.dumps(owner))
        for other in (twin, back):
            other_tm = getattr(other, 'transformer_model', other)
            assert not other_tm.__dict__.get(plans._ATTR) and torch.equal(other_tm.CLS, tm.CLS)
    assert '_aloe_train_model' not in tm.__dict__
    assert train._aloe_model_cached(tm, 1, 2, 4) is not a and built[-1] == (1, 2, 4)          # another geometry
    b = train._aloe_model_cached(tm, 1, 2, 4)
    tm.CLS.data = tm.CLS.data.clone()                                                          # a parameter moved
    assert train._aloe_model_cached(tm, 1, 2, 4) is not b and len(built) == 3
    plans.invalidate(model)
    assert not tm.__dict__.get(plans._ATTR)
    train._aloe_model_cached(tm, 1, 2, 4)
    assert len(built) == 4


def test_forward_in_train_mode_still_raises():
    from slotformer_amd import clevrer_vqa
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel, CLEVRERAloe
    tm = CLEVRERTransformerModel(*[dict(c) for c in fc.train_case(fc.CASES[0])['cfg']])
    model = CLEVRERAloe(tm).train()
    with pytest.raises(NotImplementedError, match='backward of the Aloe reasoner .* not built'):
        model({'cls_q_tokens': torch.zeros(1, 4)})
    with pytest.raises(NotImplementedError, match='backward of the Aloe reasoner .* not built'):
        tm.answer(torch.zeros(1, 1, 1, 32), torch.zeros(1, 4), torch.zeros(1, 4), False)
    with pytest.raises(NotImplementedError):
        clevrer_vqa.build_method()


def test_fit_validates_on_the_host():
    from slotformer_amd import clevrer_vqa
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel, CLEVRERAloe
    cfg, sd, slots, q = fc.fit_case()
    model = CLEVRERAloe(CLEVRERTransformerModel(*[dict(c) for c in cfg]))
    slots = torch.from_numpy(slots)
    with pytest.raises(ValueError, match=r'slots are a \[V, T, N, 32\]'):
        clevrer_vqa.fit(model, slots[..., :16], q, 1)
    with pytest.raises(ValueError, match='batch_size >= 1'):
        clevrer_vqa.fit(model, slots, q, 1, batch_size=0)
    with pytest.raises(IndexError, match='cls_video_index'):
        clevrer_vqa.fit(model, slots[:8], q, 1)
    with pytest.raises(IndexError, match='mc_start'):
        clevrer_vqa.fit(model, slots, dict(q, mc_start=q['mc_start'] + 1), 1)
    with pytest.raises(ValueError, match='non-decreasing'):
        clevrer_vqa.fit(model, slots, dict(q, mc_flag=q['mc_flag'][::-1]), 1)
    with pytest.raises(ValueError, match='cls_video_index is missing'):
        clevrer_vqa.fit(model, slots, {k: v for k, v in q.items() if k != 'cls_video_index'}, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clevrer_vqa.fit(model, slots, q, 1)
    with pytest.raises(ValueError, match='batch_size >= 1'):
        clevrer_vqa.evaluate(model, slots, q, batch_size=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clevrer_vqa.evaluate(model, slots, q)


def test_collated_arrays_treat_each_kind_on_its_own():
    from slotformer_amd import clevrer_vqa
    hc = cases.harness_case()[3]                          # 5 descriptive questions, 4 multiple-choice ones with 3, 1, 4, 2 choices
    q = dict(hc, cls_label=np.arange(5), mc_label=np.zeros(10, np.float32))
    cpu = torch.device('cpu')
    flag = np.asarray(q['mc_flag'])
    full = clevrer_vqa._collated(q, cpu)
    assert full['video'].tolist() == list(q['cls_video_index']) + list(np.asarray(q['mc_video_index'])[flag])
    assert full['start'].tolist() == list(q['cls_start']) + list(np.asarray(q['mc_start'])[flag])
    no_mc_start = clevrer_vqa._collated({k: v for k, v in q.items() if k != 'mc_start'}, cpu)   # a missing array of one kind leaves the other alone
    assert no_mc_start['start'].tolist() == list(q['cls_start']) + [0] * 10
    no_cls_start = clevrer_vqa._collated({k: v for k, v in q.items() if k != 'cls_start'}, cpu)
    assert no_cls_start['start'].tolist() == [0] * 5 + list(np.asarray(q['mc_start'])[flag])
    for kind in ('cls', 'mc'):
        with pytest.raises(ValueError, match=f'{kind}_video_index is missing'):
            clevrer_vqa._collated({k: v for k, v in q.items() if k != f'{kind}_video_index'}, cpu)
    only_cls = clevrer_vqa._collated({k: v for k, v in q.items() if not k.startswith('mc_')}, cpu)
    assert only_cls['video'].tolist() == list(q['cls_video_index']) and only_cls['qn'] == 0 and only_cls['tokens'].shape == (5, 32)


def test_schedule_draws_every_question_once_per_epoch():
    from slotformer_amd import clevrer_vqa, physion_vqa, phyre_planning
    assert clevrer_vqa.step_seed is physion_vqa.step_seed is phyre_planning.step_seed and clevrer_vqa.batch_schedule is physion_vqa.batch_schedule
    assert clevrer_vqa.step_seed(5, 7) == (5 << 32) | 7
    hc = cases.harness_case()[3]                          # 5 descriptive questions, 4 multiple-choice ones with 3, 1, 4, 2 choices
    a, b = clevrer_vqa.question_schedule(hc, 3, 4, 5), clevrer_vqa.question_schedule(hc, 3, 4, 5)
    flat = lambda s: [[{k: v.tolist() for k, v in bt.items()} for bt in e] for e in s]  # noqa: E731
    assert flat(a) == flat(b) and flat(a) != flat(clevrer_vqa.question_schedule(hc, 3, 4, 6))
    first = np.searchsorted(hc['mc_flag'], np.arange(4))
    for e in a:
        assert [len(bt['cls']) + len(bt['mc']) for bt in e] == [4, 4, 1]          # questions, not sequences
        assert sorted(i for bt in e for i in bt['cls'].tolist()) == list(range(5))
        assert sorted(i for bt in e for i in bt['mc'].tolist()) == list(range(4))
        assert sorted(i for bt in e for i in bt['mc_rows'].tolist()) == list(range(10))
        for bt in e:   # the choices of a question stand together, in order, in the order the questions were drawn
            want = [r for qn in bt['mc'] for r in range(first[qn], first[qn] + [3, 1, 4, 2][qn])]
            assert bt['mc_rows'].tolist() == want
    assert flat(a)[0] != flat(a)[1]
    only_cls = {k: v for k, v in hc.items() if not k.startswith('mc_')}
    assert all(len(bt['mc_rows']) == 0 for e in clevrer_vqa.question_schedule(only_cls, 1, 2, 0) for bt in e)
    with pytest.raises(ValueError, match='no question'):
        clevrer_vqa.question_schedule({}, 1, 2, 0)


def test_fit64_learns_the_planted_set():
    cfg, sd, slots, q = fc.fit_case()
    f = fc.FIT
    _, losses = fc.fit64(cfg, sd, slots, q, f['epochs'], f['batch_size'], f['lr'], f['seed'])
    total = losses.sum(-1)
    print('float64 fit: epoch losses (CE + BCE) first', total[0], 'last', total[-1], 'ratio', total[-1] / total[0])
    assert np.isfinite(losses).all() and total[-1] < 0.25 * total[0]
