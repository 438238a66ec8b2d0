"""CPU: what the workspace queries return whose layout is one carve over csrc/sf_arena.h (the query runs it over a NULL base, the call over the
caller's buffer).  tests/golden/workspace_bytes.json holds every value of `record(lib)` as the library of commit 4d05598 returned it -- the last
commit in which each of these queries was a sum written by hand next to the pointer walk of its call -- through
`SF_LIB_PATH=<that build> python tools/gen_golden_workspace_bytes.py`; never regenerate it from the tree under test.

Per query: the reference configurations of configs.py, the smallest accepted arguments, arguments whose buffers are no multiple of 64 floats (the
rounding shows) and a refused set, which returns 0.  The models carry dummy non-null weight pointers: a query reads shapes and which pointers are
there, never a weight.  Every query here runs without a device."""
import ctypes as C
import json
import os

import pytest

from slotformer_amd import configs

DUMMY = 0x1000   # never dereferenced
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_bytes.json')
# (M, N, K) of LINEAR_CASES in tests/test_train_kernels_gpu.py (a GPU module: not imported here; test_linear_shapes_are_the_gpu_tests checks the copy)
LINEAR_SHAPES = [(7, 64, 64), (64, 256, 256), (1060, 768, 256), (1000, 64, 64), (49152, 64, 64), (49157, 192, 192), (1344, 1024, 256), (1344, 768, 256),
                 (50000, 576, 192)]


def _fill(m, skip=()):
    """every pointer field of a ctypes model DUMMY (arrays of pointers too), except the names in `skip`"""
    from slotformer_amd import _lib
    for f, t in m._fields_:
        if f in skip:
            continue
        if t is _lib.FP or t is C.c_void_p:
            setattr(m, f, DUMMY)
        elif isinstance(t, type) and issubclass(t, C.Array) and t._type_ is C.c_void_p:
            for i in range(t._length_):
                getattr(m, f)[i] = DUMMY
    return m


def rollouter(num_slots, slot_size, window, d_model, layers, heads, ffn, single_step=0, with_layers=True, norm_first=1):
    from slotformer_amd import _lib
    m = _fill(_lib.sf_rollouter())
    m.num_slots, m.slot_size, m.d_model, m.num_layers, m.num_heads, m.ffn_dim = num_slots, slot_size, d_model, layers, heads, ffn
    m.norm_first, m.window_len, m.single_step = norm_first, window, single_step
    keep = (_lib.sf_tfm_layer * layers)()
    if with_layers:
        m.layers = keep
    return m, keep


def cfg_rollouter(cfg):
    rd = cfg['rollout_dict']
    single = cfg['model'] == 'SingleStepSlotFormer'
    return rollouter(rd['num_slots'], rd['slot_size'], rd['cond_len'] if single else rd['history_len'], rd['d_model'], rd['num_layers'],
                     rd['num_heads'], rd['ffn_dim'], single_step=int(single))


def slot_attention(in_features, slot_size, mlp_hidden, num_slots):
    from slotformer_amd import _lib
    m = _fill(_lib.sf_slot_attention())
    m.in_features, m.slot_size, m.mlp_hidden, m.num_slots, m.eps = in_features, slot_size, mlp_hidden, num_slots, 1e-6
    return m


def savi_features(resolution, hidden, out_channels, layers=4, channels=64, ks=5):
    from slotformer_amd import _lib
    m = _fill(_lib.sf_savi_features())
    m.resolution, m.layers, m.channels, m.ks, m.hidden, m.out_channels = resolution, layers, channels, ks, hidden, out_channels
    return m


def savi_decoder(resolution, num_slots, slot_size=128, dec_res=8, channels=(64, 64, 64, 64), ks=5):
    """the reference decoder: stride-2 transposed convolutions up to the resolution, stride 1 from there"""
    from slotformer_amd import _lib
    m = _fill(_lib.sf_savi_decoder())
    m.resolution, m.dec_layers, m.dec_ks, m.dec_res, m.num_slots, m.slot_size = resolution, len(channels), ks, dec_res, num_slots, slot_size
    size = dec_res
    for i, c in enumerate((slot_size,) + tuple(channels)):
        m.dec_channels[i] = c
    for i in range(len(channels)):
        m.dec_strides[i] = 2 if size < resolution else 1
        size *= m.dec_strides[i]
    return m


def phyre_model(num_slots, slot_size=128, layers=4, d_model=128, heads=8, ffn=512):
    from slotformer_amd import _lib
    m = _fill(_lib.sf_phyre_readout_model())
    m.num_slots, m.slot_size, m.d_model, m.num_heads, m.ffn_dim, m.num_layers = num_slots, slot_size, d_model, heads, ffn, layers
    keep = (_lib.sf_tfm_layer * max(layers, 1))()
    m.layers = keep
    return m, keep


def slate_decoder(d_model, heads, layers, vocab, num_slots, max_len):
    from slotformer_amd import _lib
    m = _fill(_lib.sf_slate_decoder())
    m.d_model, m.num_heads, m.num_layers, m.vocab_size, m.num_slots, m.max_len = d_model, heads, layers, vocab, num_slots, max_len
    keep = (_lib.sf_slate_block * max(layers, 1))()
    m.blocks = keep
    return m, keep


def record(lib):
    """{key: bytes} of every pinned query; the same function produced the golden file from the parent commit's library"""
    r = {}

    # ---- rollout training: reference rollouters (windowed C1 / C2 / C4 and its 15-frame reference window, single-step C5), the training fixture ----
    rolls = {'c1': cfg_rollouter(configs.C1_ROLL), 'c2': cfg_rollouter(configs.C2_ROLL), 'c4': cfg_rollouter(configs.C4_ROLL),
             'c4_ref': cfg_rollouter(configs.C4_ROLL_REF), 'c5_single': cfg_rollouter(configs.C5_ROLL), 'train': cfg_rollouter(configs.TRAIN_ROLL),
             'min': rollouter(1, 64, 1, 64, 1, 1, 64), 'odd': rollouter(3, 64, 5, 64, 1, 2, 192),   # 15-token windows: rows no multiple of 64
             'odd_single': rollouter(5, 64, 3, 128, 2, 4, 128, single_step=1)}
    for name, (m, _) in rolls.items():
        for B in (1, 3, 64):
            for S in (1, 6, 10):
                r['rollout_train/%s/B%d/S%d' % (name, B, S)] = lib.sf_rollout_train_workspace_bytes(C.byref(m), B, S)
    refused = {'no_layers': rollouter(6, 128, 6, 128, 4, 8, 512, with_layers=False), 'post_norm': rollouter(6, 128, 6, 128, 4, 8, 512, norm_first=0),
               'd_100': rollouter(6, 128, 6, 100, 4, 4, 512), 'window_132': rollouter(6, 128, 22, 128, 4, 8, 512), 'layers_17': rollouter(6, 128, 6, 128, 17, 8, 512)}
    for name, (m, _) in refused.items():
        r['rollout_train/refused_%s' % name] = lib.sf_rollout_train_workspace_bytes(C.byref(m), 2, 3)
    r['rollout_train/refused_B0'] = lib.sf_rollout_train_workspace_bytes(C.byref(rolls['c1'][0]), 0, 3)
    r['rollout_train/refused_null'] = lib.sf_rollout_train_workspace_bytes(None, 2, 3)

    # ---- Slot Attention training ----
    sas = {'c1': slot_attention(128, 128, 256, 6), 'c4': slot_attention(192, 192, 384, 6), 'n7': slot_attention(128, 128, 256, 7),
           'n11': slot_attention(128, 128, 256, 11), 'n16': slot_attention(128, 128, 256, 16), 'min': slot_attention(64, 64, 64, 1)}
    for name, m in sas.items():
        for B in (1, 3):
            for HW in (1024, 4096):
                for it in (1, 2, 3):
                    r['slot_attention_train/%s/B%d/HW%d/it%d' % (name, B, HW, it)] = lib.sf_slot_attention_train_workspace_bytes(C.byref(m), B, HW, it)
    r['slot_attention_train/min/B1/HW16/it1'] = lib.sf_slot_attention_train_workspace_bytes(C.byref(sas['min']), 1, 16, 1)
    r['slot_attention_train/refused_17_slots'] = lib.sf_slot_attention_train_workspace_bytes(C.byref(slot_attention(128, 128, 256, 17)), 1, 1024, 2)
    r['slot_attention_train/refused_slot_size_96'] = lib.sf_slot_attention_train_workspace_bytes(C.byref(slot_attention(128, 96, 256, 6)), 1, 1024, 2)
    r['slot_attention_train/refused_9_iterations'] = lib.sf_slot_attention_train_workspace_bytes(C.byref(sas['c1']), 1, 1024, 9)
    r['slot_attention_train/refused_HW_1000'] = lib.sf_slot_attention_train_workspace_bytes(C.byref(sas['c1']), 1, 1000, 2)
    for B, HW, N, D in ((1, 16, 1, 64), (1, 1024, 6, 128), (3, 4096, 7, 128), (5, 4096, 11, 192), (2, 1000, 16, 256), (64, 4096, 8, 128)):
        r['slot_attn_iter_bwd/B%d/HW%d/N%d/D%d' % (B, HW, N, D)] = lib.sf_slot_attn_iter_bwd_workspace_bytes(B, HW, N, D)
        r['slot_attn_iter_bwd16/B%d/HW%d/N%d/D%d' % (B, HW, N, D)] = lib.sf_slot_attn_iter_bwd16_workspace_bytes(B, HW, N, D)

    # ---- SAVi encoder features / decoder training ----
    feats = {'c1': savi_features(64, 128, 128), 'c2': savi_features(128, 128, 128), 'c4': savi_features(128, 192, 192), 'min': savi_features(64, 64, 64, layers=2),
             'wide': savi_features(64, 1024, 64, layers=8)}
    for name, m in feats.items():
        for F in (1, 5, 24):
            r['savi_features_train/%s/F%d' % (name, F)] = lib.sf_savi_features_train_workspace_bytes(C.byref(m), F)
    r['savi_features_train/refused_res_96'] = lib.sf_savi_features_train_workspace_bytes(C.byref(savi_features(96, 128, 128)), 1)
    r['savi_features_train/refused_32_channels'] = lib.sf_savi_features_train_workspace_bytes(C.byref(savi_features(64, 128, 128, channels=32)), 1)
    r['savi_features_train/refused_hidden_100'] = lib.sf_savi_features_train_workspace_bytes(C.byref(savi_features(64, 100, 128)), 1)
    r['savi_features_train/refused_F0'] = lib.sf_savi_features_train_workspace_bytes(C.byref(feats['c1']), 0)
    for F in (1, 7, 4096, 0, 4097):
        r['conv_first_wgrad/F%d' % F] = lib.sf_conv_first_wgrad_workspace_bytes(F)
    decs = {'c1': savi_decoder(64, 6), 'c2': savi_decoder(128, 7), 'c4': savi_decoder(128, 6, slot_size=192), 'c5': savi_decoder(128, 8, dec_res=16),
            'min': savi_decoder(8, 1, slot_size=4, dec_res=8, channels=(4,), ks=1), 'odd': savi_decoder(20, 3, slot_size=12, dec_res=5, channels=(20, 12), ks=3)}
    for name, m in decs.items():
        for F in (1, 3):
            r['savi_decode_train/%s/F%d' % (name, F)] = lib.sf_savi_decode_train_workspace_bytes(C.byref(m), F)
            r['savi_decode/%s/F%d' % (name, F)] = lib.sf_savi_decode_workspace_bytes(C.byref(m), F)
    r['savi_decode/c2/F100'] = lib.sf_savi_decode_workspace_bytes(C.byref(decs['c2']), 100)   # more than one chunk of frames
    bad = savi_decoder(64, 6)
    bad.resolution = 96
    r['savi_decode_train/refused_size_mismatch'] = lib.sf_savi_decode_train_workspace_bytes(C.byref(bad), 1)
    r['savi_decode_train/refused_even_kernel'] = lib.sf_savi_decode_train_workspace_bytes(C.byref(savi_decoder(64, 6, ks=4)), 1)
    r['savi_decode_train/refused_F0'] = lib.sf_savi_decode_train_workspace_bytes(C.byref(decs['c1']), 0)
    r['savi_decode/refused_F0'] = lib.sf_savi_decode_workspace_bytes(C.byref(decs['c1']), 0)
    for Cl in (4, 12, 32, 64, 0, 6, 68):
        r['savi_decode_head_bwd/Cl%d' % Cl] = lib.sf_savi_decode_head_bwd_workspace_bytes(Cl)

    # ---- PHYRE readout training: 1 + T N in {2, 37, 91} ----
    for N, T in ((1, 1), (6, 6), (9, 10), (8, 6)):
        for nl in (1, 4, 8):
            m, _ = phyre_model(N, layers=nl)
            for B in (1, 5, 64):
                r['phyre_readout_train/N%d/T%d/layers%d/B%d' % (N, T, nl, B)] = lib.sf_phyre_readout_train_workspace_bytes(C.byref(m), B, T)
    r['phyre_readout_train/refused_97_tokens'] = lib.sf_phyre_readout_train_workspace_bytes(C.byref(phyre_model(8)[0]), 2, 12)
    r['phyre_readout_train/refused_d_256'] = lib.sf_phyre_readout_train_workspace_bytes(C.byref(phyre_model(8, d_model=256)[0]), 2, 6)
    r['phyre_readout_train/refused_9_layers'] = lib.sf_phyre_readout_train_workspace_bytes(C.byref(phyre_model(8, layers=9)[0]), 2, 6)
    r['phyre_readout_train/refused_B0'] = lib.sf_phyre_readout_train_workspace_bytes(C.byref(phyre_model(8)[0]), 0, 6)

    # ---- the differentiable building blocks ----
    for M, N, K in LINEAR_SHAPES + [(1, 64, 64), (1000000, 1024, 256), (64, 3072, 1024)]:
        r['linear_bwd/M%d/N%d/K%d' % (M, N, K)] = lib.sf_linear_bwd_workspace_bytes(M, N, K)
    for D in (4, 260, 1024, 64, 1):
        r['layernorm_bwd/D%d' % D] = lib.sf_layernorm_bwd_workspace_bytes(D)
    for F in (1, 3):
        for HW in (8, 64):
            for Cn in (64, 128, 192):   # (below 64 channels the query of 4d05598 divides by zero: its weight-gradient tiles are 64 wide)
                r['groupnorm1_bwd/F%d/H%d/C%d' % (F, HW, Cn)] = lib.sf_groupnorm1_bwd_workspace_bytes(F, HW, HW, Cn)
    r['groupnorm1_bwd/F2/H5x3/C64'] = lib.sf_groupnorm1_bwd_workspace_bytes(2, 5, 3, 64)
    r['groupnorm1_bwd/refused_F0'] = lib.sf_groupnorm1_bwd_workspace_bytes(0, 8, 8, 16)
    r['groupnorm1_bwd/refused_C0'] = lib.sf_groupnorm1_bwd_workspace_bytes(1, 8, 8, 0)
    r['groupnorm1_bwd/refused_H0'] = lib.sf_groupnorm1_bwd_workspace_bytes(1, 0, 8, 64)
    for B, Lq, H in ((1, 1, 1), (3, 17, 4), (12, 1024, 4), (64, 257, 8)):
        r['slate_attention_bwd/B%d/Lq%d/H%d' % (B, Lq, H)] = lib.sf_slate_attention_bwd_workspace_bytes(B, Lq, H)

    # ---- STEVE's token generation: the launch chain and the one-launch-per-token form (sf_slate_step_ok) ----
    slates = {'physion': slate_decoder(256, 4, 8, 4096, 6, 1024), 'reduced': slate_decoder(64, 4, 2, 64, 4, 256), 'min': slate_decoder(32, 1, 1, 1, 1, 0),
              'odd': slate_decoder(36, 3, 3, 77, 5, 64),          # d_model no multiple of 32: the chain only
              'layers9': slate_decoder(64, 4, 9, 64, 4, 256),     # more blocks than the one-launch form holds
              'layers17': slate_decoder(64, 4, 17, 64, 4, 256)}   # more than the chain itself accepts: the query still counts them
    for name, (m, _) in slates.items():
        r['slate_step_ok/%s' % name] = lib.sf_slate_step_ok(C.byref(m))
        for B in (1, 12, 193):
            for steps in (1, 17):
                r['slate_generate/%s/B%d/steps%d' % (name, B, steps)] = lib.sf_slate_generate_workspace_bytes(C.byref(m), B, steps)
                r['slate_generate_tok/%s/B%d/steps%d' % (name, B, steps)] = lib.sf_slate_generate_tok_workspace_bytes(C.byref(m), B, steps)
    r['slate_generate/physion/B12/steps1024'] = lib.sf_slate_generate_workspace_bytes(C.byref(slates['physion'][0]), 12, 1024)
    r['slate_generate_tok/physion/B12/steps1024'] = lib.sf_slate_generate_tok_workspace_bytes(C.byref(slates['physion'][0]), 12, 1024)
    for name, args in (('null', (None, 1, 1)), ('B0', (C.byref(slates['reduced'][0]), 0, 1)), ('steps0', (C.byref(slates['reduced'][0]), 1, 0))):
        r['slate_generate/refused_%s' % name] = lib.sf_slate_generate_workspace_bytes(*args)
        r['slate_generate_tok/refused_%s' % name] = lib.sf_slate_generate_tok_workspace_bytes(*args)

    # ---- evaluation metrics ----
    for H, W, chunk in ((64, 64, 16), (128, 128, 8), (16, 16, 1), (17, 23, 3), (15, 64, 1), (64, 64, 0), (64, 64, 16385)):
        r['lpips/H%d/W%d/chunk%d' % (H, W, chunk)] = lib.sf_lpips_workspace_bytes(H, W, chunk)
    for F, H, W in ((0, 64, 64), (1, 11, 11), (7, 37, 53), (60, 64, 64), (300, 128, 128), (1, 10, 64), (-1, 64, 64)):
        r['vp_metrics/F%d/H%d/W%d' % (F, H, W)] = lib.sf_vp_metrics_workspace_bytes(F, H, W)
    return r


GROUPS = ['rollout_train', 'slot_attention_train', 'slot_attn_iter_bwd', 'slot_attn_iter_bwd16', 'savi_features_train', 'conv_first_wgrad',
          'savi_decode_train', 'savi_decode', 'savi_decode_head_bwd', 'phyre_readout_train', 'linear_bwd', 'layernorm_bwd', 'groupnorm1_bwd',
          'slate_attention_bwd', 'slate_step_ok', 'slate_generate', 'slate_generate_tok', 'lpips', 'vp_metrics']


@pytest.fixture(scope='module')
def recorded():
    """one pass over every query under the split-bf16 default (no query here reads a process switch; pinned all the same), shared by the tests"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(1)
    r = record(lib)
    lib.sf_set_precision(old)
    with open(GOLDEN) as f:
        return r, json.load(f)


@pytest.mark.parametrize('group', GROUPS)
def test_workspace_bytes(recorded, group):
    got, golden = recorded
    want = {k: v for k, v in golden.items() if k.split('/')[0] == group}
    have = {k: v for k, v in got.items() if k.split('/')[0] == group}
    assert want and sorted(want) == sorted(have), group
    wrong = {k: (have[k], want[k]) for k in want if have[k] != want[k]}
    assert not wrong, wrong


def test_every_recorded_key_is_pinned_and_grouped(recorded):
    got, golden = recorded
    assert sorted(got) == sorted(golden)
    assert {k.split('/')[0] for k in got} == set(GROUPS)


def test_refused_arguments_return_zero_and_accepted_ones_do_not(recorded):
    got, _ = recorded
    for k, v in got.items():
        if k.startswith('slate_step_ok/'):
            continue
        if '/refused_' in k:
            assert v == 0, k
    for k in ('conv_first_wgrad/F0', 'conv_first_wgrad/F4097', 'savi_decode_head_bwd/Cl0', 'savi_decode_head_bwd/Cl6', 'savi_decode_head_bwd/Cl68',
              'lpips/H15/W64/chunk1', 'lpips/H64/W64/chunk0', 'lpips/H64/W64/chunk16385', 'vp_metrics/F1/H10/W64', 'vp_metrics/F-1/H64/W64'):
        assert got[k] == 0, k
    for k in ('conv_first_wgrad/F1', 'conv_first_wgrad/F4096', 'savi_decode_head_bwd/Cl4', 'savi_decode_head_bwd/Cl64', 'rollout_train/min/B1/S1',
              'slot_attention_train/min/B1/HW16/it1', 'savi_features_train/min/F1', 'savi_decode_train/min/F1', 'phyre_readout_train/N1/T1/layers1/B1',
              'slate_generate/min/B1/steps1', 'lpips/H16/W16/chunk1', 'vp_metrics/F1/H11/W11'):
        assert got[k] > 0, k


def test_linear_shapes_are_the_gpu_tests():
    """LINEAR_SHAPES above is the (M, N, K) set of tests/test_train_kernels_gpu.py's LINEAR_CASES"""
    import test_train_kernels_gpu as t
    assert sorted(set((M, N, K) for M, N, K, _, _ in t.LINEAR_CASES)) == sorted(LINEAR_SHAPES)
