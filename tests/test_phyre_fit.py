"""CPU: the training path of the PHYRE readout without a device -- the float64 restatement of tests/phyre_fit_cases.py against the REFERENCE's
gradients (tests/golden/phyre_readout_grads.npz, tools/gen_golden_phyre_readout_grads.py), the band condition that keeps the GPU test's gate rule
honest, the ABI of the two calls and their argument errors, the host-side validation of `fit`, the schedule, the mask-index convention, and the
float64 run of the planted set that fixes the epoch count of the GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import phyre_fit_cases as fc
import phyre_readout_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_the_reference_gradients():
    loss, _, grads, _ = fc.loss_and_grads64(fc.fixture_train_case())
    worst = fc.check_against_golden(grads, loss, 1e-9)
    print(f'float64 restatement vs the reference fixture: worst relative error {worst:.2e}')


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
def test_few_gates_lie_inside_the_band(case):
    """From float64 alone: at most 1 % of a case's gates are close enough to zero for a device to decide them either way."""
    tc = fc.train_case(case)
    _, logits, grads, pre = fc.loss_and_grads64(tc)
    shares = fc.band_shares(pre)
    print(case['name'], 'share of gates inside the band per layer / head:', ['%.4f' % s for s in shares])
    assert len(pre) == case['nl'] + 1 and max(shares) <= fc.BAND_SHARE
    assert np.isfinite(logits).all() and all(np.isfinite(v).all() for v in grads.values())
    assert all(np.abs(v).max() > 0 for v in grads.values())   # every leaf is reached (a dead gradient would make a relative bound void)
    L = 1 + case['T'] * case['N']
    assert pre[0].shape == (case['B'], L, 512) and L <= 96


def test_cases_cover_the_table_of_the_issue():
    by = {c['name']: c for c in fc.CASES}
    assert [(c['B'], c['N'], c['T'], 1 + c['T'] * c['N'], c['C'], c['nl'], c['p']) for c in fc.CASES[:6]] == [
        (1, 1, 1, 2, 32, 1, 0.0), (3, 8, 2, 17, 128, 4, 0.1), (2, 16, 2, 33, 64, 2, 0.1), (2, 5, 19, 96, 32, 1, 0.1), (5, 8, 2, 17, 256, 2, 0.0),
        (9, 8, 2, 17, 128, 1, 0.1)]
    assert by['ref']['sel'] == [0, 3] and by['pad']['sel'] == [-1, 1] and by['pad']['video_index'] == (2, 0, 2, 1, 0) and by['pad']['V'] == 3
    assert by['pad']['t_pe'] == 'learnable' and by['pad']['strided']


def header_text():
    txt = open(os.path.join(ROOT, 'include', 'slotformer_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


def test_symbols_are_declared_exported_and_mirrored():
    from slotformer_amd import _lib, build
    lib = _lib.lib()
    txt = header_text()
    for name in ('sf_phyre_readout_train_workspace_bytes', 'sf_phyre_readout_train_fwd_f32', 'sf_phyre_readout_train_bwd_f32'):
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = txt[txt.index(name + '('):]
        n_args = decl[:decl.index(';')].count(',') + 1
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert 'phyre_readout_train.hip' in build.SOURCES

    def fields(name):
        end = txt.index('} ' + name + ';')
        body = txt[txt.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
        out = []
        for decl in body.split(';'):
            decl = re.sub(r'^(const\s+)?(float|int|sf_tfm_layer_grads|sf_tfm_layer)\s*', '', decl.strip())
            out += [re.sub(r'[\*\s]', '', f) for f in decl.split(',') if f.strip()]
        return out

    assert [f[0] for f in _lib.sf_phyre_readout_model._fields_] == fields('sf_phyre_readout_model')
    assert [f[0] for f in _lib.sf_phyre_readout_grads._fields_] == fields('sf_phyre_readout_grads')
    assert C.sizeof(_lib.sf_phyre_readout_model) == 6 * 4 + 9 * 8 and C.sizeof(_lib.sf_phyre_readout_grads) == 9 * 8


def dummy_model(N=8, Cs=128, nl=4, ptr=4096):
    """a descriptor whose device pointers are a non-null, aligned dummy: every case below is refused before one is dereferenced"""
    from slotformer_amd import _lib
    m = _lib.sf_phyre_readout_model()
    m.num_slots, m.slot_size, m.d_model, m.num_heads, m.ffn_dim, m.num_layers = N, Cs, 128, 8, 512, nl
    for f in ('in_proj_w', 'in_proj_b', 'enc_t_pe', 'cls', 'mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2'):
        setattr(m, f, ptr)
    arr = (_lib.sf_tfm_layer * max(nl, 1))()
    for layer in arr:
        for f, _ in _lib.sf_tfm_layer._fields_[:12]:
            setattr(layer, f, ptr)
    m.layers = C.cast(arr, C.POINTER(_lib.sf_tfm_layer))
    g = _lib.sf_phyre_readout_grads()
    for f in ('in_proj_w', 'in_proj_b', 'enc_t_pe', 'cls', 'mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2'):
        setattr(g, f, ptr)
    garr = (_lib.sf_tfm_layer_grads * max(nl, 1))()
    for layer in garr:
        for f, _ in _lib.sf_tfm_layer_grads._fields_:
            setattr(layer, f, ptr)
    g.layers = C.cast(garr, C.POINTER(_lib.sf_tfm_layer_grads))
    return m, g, (arr, garr)


def test_argument_errors_without_a_gpu():
    from slotformer_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.sf_last_error_string().decode()  # noqa: E731
    one = C.c_void_p(4096)
    m, g, keep = dummy_model()
    q = lib.sf_phyre_readout_train_workspace_bytes
    assert q(C.byref(m), 256, 2) > 0 and q(C.byref(m), 0, 2) == 0 and q(C.byref(m), 4, 12) == 0 and q(None, 4, 2) == 0
    for odd in (dict(N=17), dict(Cs=100), dict(nl=9), dict(nl=0)):
        assert q(C.byref(dummy_model(**odd)[0]), 4, 2) == 0, odd
    assert q(C.byref(m), 256, 2) > q(C.byref(m), 64, 2)
    big = 1 << 40
    sel = (C.c_int * 2)(0, 3)

    def fwd(model=m, slots=one, sv=4 * 8 * 128, st=8 * 128, V=4, T_all=4, vi=None, s=sel, B=3, T=2, p=0.1, logits=one, ws=one, nbytes=big):
        return lib.sf_phyre_readout_train_fwd_f32(C.byref(model) if model is not None else None, slots, sv, st, V, T_all, vi, s, B, T, p, 7, logits, None,
                                                  None, ws, nbytes, None)

    def bwd(model=m, slots=one, s=sel, B=3, T=2, p=0.1, gl=one, grads=g, ws=one, nbytes=big, T_all=4):
        return lib.sf_phyre_readout_train_bwd_f32(C.byref(model), slots, 4 * 8 * 128, 8 * 128, 4, T_all, None, s, B, T, gl, C.byref(grads) if grads else None,
                                                  p, 7, ws, nbytes, None)

    old = lib.sf_get_precision()
    try:
        lib.sf_set_precision(1)
        for call in (fwd, bwd):
            assert call(slots=None) < 0 and 'null pointer' in err()
            assert call(ws=None) < 0 and 'null pointer' in err()
            assert call(T=12) < 0 and 'unsupported shape' in err()
            assert call(model=dummy_model(Cs=100)[0]) < 0 and 'unsupported shape' in err()
            assert call(s=(C.c_int * 2)(0, 4)) < 0 and 'sel[t]' in err()
            assert call(s=(C.c_int * 2)(-2, 1)) < 0 and 'sel[t]' in err()
            assert call(B=0) < 0 and 'B >= 1' in err()
            assert call(B=5) < 0 and 'video_index' in err()
            assert call(p=1.0) < 0 and 'dropout_p' in err()
            assert call(slots=C.c_void_p(4100)) < 0 and '16-byte aligned' in err()
            assert call(ws=C.c_void_p(4104)) < 0 and '16-byte aligned' in err()
            assert call(nbytes=q(C.byref(m), 3, 2) - 1) < 0 and 'workspace too small' in err()
            assert call(model=dummy_model(ptr=4100)[0]) < 0 and '16-byte aligned' in err()
            lib.sf_set_precision(0)
            assert call() < 0 and 'split-bf16' in err()
            lib.sf_set_precision(1)
        assert fwd(model=None) < 0 and fwd(logits=None) < 0 and 'null pointer' in err()
        assert fwd(st=8 * 128 - 4) < 0 and 'stride' in err()
        assert bwd(gl=None) < 0 and 'null pointer' in err()
        assert bwd(grads=None) < 0 and 'null pointer' in err()
        bad = dummy_model()[1]
        bad.cls = None
        assert bwd(grads=bad) < 0 and 'null pointer' in err()
        odd_g = dummy_model()[1]
        odd_g.layers[1].lin1_b = 4100
        assert bwd(grads=odd_g) < 0 and '16-byte aligned' in err()
    finally:
        lib.sf_set_precision(old)
    del keep


def test_fit_validates_on_the_host():
    from slotformer_amd import phyre_planning
    from slotformer_amd.phyre_planning.models import PHYREReadout
    m = PHYREReadout()
    slots = torch.zeros(6, 4, 8, 128)
    with pytest.raises(ValueError, match='6 videos, 5 labels'):
        phyre_planning.fit(m, slots, torch.zeros(5), 1)
    with pytest.raises(ValueError, match=r'slots are a \[V, T, 8, 128\]'):
        phyre_planning.fit(m, torch.zeros(6, 4, 8, 64), torch.zeros(6), 1)
    with pytest.raises(IndexError, match='frame table'):
        phyre_planning.fit(m, slots[:, :3], torch.zeros(6), 1)          # sel_slots [0, 3] on three frames
    with pytest.raises(IndexError, match='frame table'):
        phyre_planning.fit(m, slots, torch.zeros(6), 1, sel=[0, 1, 2])
    with pytest.raises(ValueError, match='batch_size >= 1'):
        phyre_planning.fit(m, slots, torch.zeros(6), 1, batch_size=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        phyre_planning.fit(m, slots, torch.zeros(6), 1)
    with pytest.raises(ValueError, match='batch_size >= 1'):
        phyre_planning.evaluate(m, slots, torch.zeros(6), batch_size=0)
    with pytest.raises(ValueError, match='6 videos, 5 labels'):
        phyre_planning.evaluate(m, slots, torch.zeros(5))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        phyre_planning.evaluate(m, slots, torch.zeros(6))


def test_schedule_is_deterministic_and_shared():
    from slotformer_amd import phyre_planning, physion_vqa
    assert phyre_planning.batch_schedule is physion_vqa.batch_schedule
    a, b = phyre_planning.batch_schedule(64, 3, 16, 5), phyre_planning.batch_schedule(64, 3, 16, 5)
    assert [[t.tolist() for t in e] for e in a] == [[t.tolist() for t in e] for e in b]
    assert [[t.tolist() for t in e] for e in a] != [[t.tolist() for t in e] for e in phyre_planning.batch_schedule(64, 3, 16, 6)]
    for e in a:
        assert sorted(int(i) for t in e for i in t) == list(range(64)) and [t.numel() for t in e] == [16] * 4
    assert [t.numel() for t in phyre_planning.batch_schedule(10, 1, 4, 0)[0]] == [4, 4, 2]
    assert phyre_planning.step_seed(5, 7) == (5 << 32) | 7 and phyre_planning.step_seed(5, 7) != phyre_planning.step_seed(7, 5)


def test_mask_index_convention():
    """The element indices the kernels use -- site 0: ((b 8 + h) L + i) L + j; sites 1, 3: (b L + tok) 128 + c; site 2: (b L + tok) 512 + j --
    are the flat indices of the restatement's mask tensors, and the masks are `train.dropout_keep_mask`'s."""
    from slotformer_amd import train
    B, L, seed, p = 3, 17, 987654321012345, 0.1
    masks = fc.keep_masks(seed, p, B, L, 2)
    scale = 1.0 / (1.0 - float(np.float32(p)))
    layer = 1
    flat0 = train.dropout_keep_mask(seed, 0, layer, 0, B * 8 * L * L, p)
    flat1 = train.dropout_keep_mask(seed, 0, layer, 1, B * L * 128, p)
    flat2 = train.dropout_keep_mask(seed, 0, layer, 2, B * L * 512, p)
    flat3 = train.dropout_keep_mask(seed, 0, layer, 3, B * L * 128, p)
    for b, h, i, j in ((0, 0, 0, 0), (2, 7, 16, 16), (1, 3, 5, 11)):
        assert float(masks[layer][0][b, h, i, j]) == scale * flat0[((b * 8 + h) * L + i) * L + j]
    for b, tok, c in ((0, 0, 0), (2, 16, 127), (1, 9, 64)):
        assert float(masks[layer][1][b, tok, c]) == scale * flat1[(b * L + tok) * 128 + c]
        assert float(masks[layer][3][b, tok, c]) == scale * flat3[(b * L + tok) * 128 + c]
        assert float(masks[layer][2][b, tok, 4 * c + 3]) == scale * flat2[(b * L + tok) * 512 + 4 * c + 3]
    assert not np.array_equal(flat1, flat3) and abs(flat2.mean() - 0.9) < 0.01
    assert fc.keep_masks(seed, 0.0, B, L, 2) is None


def test_training_mode_forward_and_build_method_still_raise():
    from slotformer_amd import phyre_planning
    from slotformer_amd.phyre_planning.models import PHYREReadout
    m = PHYREReadout()
    with pytest.raises(NotImplementedError, match='not built'):
        m({'slots': torch.zeros(2, 4, 8, 128)})
    with pytest.raises(NotImplementedError, match='training kernels of this readout .* not built'):
        m.logits_of(torch.zeros(2, 4, 8, 128))
    with pytest.raises(NotImplementedError):
        phyre_planning.build_method()


def test_parameter_order_is_the_gradient_layout():
    from slotformer_amd import ops, train
    from slotformer_amd.phyre_planning.models import PHYREReadout
    for t_pe in ('sin', 'learnable'):
        rd = dict(cases.readout_dict(4, 32, (0, 1), 2), t_pe=t_pe)
        m = PHYREReadout(rd)
        ps = train.phyre_readout_parameters(m)
        layout = ops.phyre_grad_layout(32, 2, 2, t_pe == 'learnable')
        assert [p.numel() for p in ps] == [k for _, k in layout]
        names = {id(p): n for n, p in m.named_parameters()}
        assert [names[id(p)] for p in ps] == fc.grad_keys(rd, t_pe == 'learnable')
        assert all(p.requires_grad for p in ps)
        offs = np.cumsum([0] + [k for _, k in layout])[:-1]
        assert all(o % 4 == 0 for o in offs)   # every leaf of the flat bucket starts 16-byte aligned


def test_float64_fit_separates_the_planted_set():
    """The epoch count of the GPU fit test is chosen here: the float64 run of the same schedule, masks, Adam and learning-rate rule classifies
    the 64 planted videos with every |logit| > 1."""
    rd, sd, slots, labels = fc.fit_case()
    assert 0.3 < labels.mean() < 0.7
    f = fc.FIT
    w, losses = fc.fit64(rd, sd, slots, labels, f['epochs'], f['batch_size'], f['lr'], f['seed'], f['warmup'])
    logits, _ = fc.forward64(w, rd, slots, rd['sel_slots'])
    logits = logits.numpy()
    print('float64 fit: losses', ['%.4f' % v for v in losses], 'min |logit| %.3f' % np.abs(logits).min())
    assert ((logits > 0) == (labels > 0.5)).all() and np.abs(logits).min() > 1.0
    assert np.isfinite(losses).all() and losses[-1] < 0.1 * losses[0]
