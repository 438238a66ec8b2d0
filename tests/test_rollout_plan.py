"""CPU: the rollout's plan as the C ABI reports it (sf_rollout_is_fused, sf_rollout_tok_ok, sf_rollout_uses_seam[_opts],
sf_rollout_workspace_bytes) for the rollouters of configs.py.  The rollouters carry dummy non-null weight pointers: the plan reads
which packed copies are there, never a weight."""
import ctypes as C

import pytest

from slotformer_amd import configs

DUMMY = 0x1000   # never dereferenced


def rollouter(cfg, window=None, null_tok_layer=None):
    from slotformer_amd import _lib
    rd = cfg['rollout_dict']
    nl = rd['num_layers']
    layers = (_lib.sf_tfm_layer * nl)()
    for i, layer in enumerate(layers):
        for f, _ in _lib.sf_tfm_layer._fields_:
            setattr(layer, f, None if (f == 'tok_packed' and i == null_tok_layer) else DUMMY)
    single = 'cond_len' in rd
    W = window or (rd['cond_len'] if single else rd['history_len'])
    m = _lib.sf_rollouter(rd['num_slots'], rd['slot_size'], rd['d_model'], nl, rd['num_heads'], rd['ffn_dim'], int(rd['norm_first']), W,
                          int(single))
    for f in ('in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'pe_tok', 'in_proj_packed', 'out_proj_packed'):
        setattr(m, f, DUMMY)
    m.layers = C.cast(layers, C.POINTER(_lib.sf_tfm_layer))
    m._layers = layers   # keeps the array alive
    return m


SHAPES = {
    'c2': (configs.C2_ROLL, None),                # d 256, 7 slots x 6 frames: fused layers on the projection ring
    'c4': (configs.C4_ROLL, None),                # slot size 192: fused layers, no ring
    'c4_ref': (configs.C4_ROLL_REF, None),        # 15 frames x 6 slots = 90 tokens: the long-window path
    'c1': (configs.C1_ROLL, None),                # d 128: generic GEMM layers
    'c5': (configs.C5_ROLL, None),                # single-step rollouter, window growing to 6 x 8 slots
    'c2_4x7': (configs.C2_ROLL, 4),               # 28 tokens: no window a seam launch accepts
}


@pytest.fixture
def lib():
    """Process defaults the plan depends on: split-bf16, token-stationary layers off, seams on -- restored afterwards."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision(), lib.sf_get_layer_tok(), lib.sf_get_seam_fused()
    lib.sf_set_precision(1)
    lib.sf_set_layer_tok(0)
    lib.sf_set_seam_fused(1)
    yield lib
    lib.sf_set_precision(old[0])
    lib.sf_set_layer_tok(old[1])
    lib.sf_set_seam_fused(old[2])


def opts(**kw):
    from slotformer_amd import _lib
    o = dict(precision=-1, seam_fused=-1, ffn_rows=0, attn_heads_per_wg=0, attn_qkv_rows=0, ffn_tile=0, cus_available=0, layer_tok=0)
    o.update(kw)
    return _lib.sf_rollout_opts(**o)


def uses_seam(lib, m, B, **kw):
    return lib.sf_rollout_uses_seam_opts(C.byref(m), B, C.byref(opts(**kw)))


@pytest.mark.parametrize('name,fused,tok', [('c2', 1, 1), ('c4', 1, 1), ('c4_ref', 0, 0), ('c1', 0, 0), ('c5', 1, 1), ('c2_4x7', 1, 1)])
def test_fused_and_tok_per_shape(lib, name, fused, tok):
    m = rollouter(*SHAPES[name])
    assert lib.sf_rollout_is_fused(C.byref(m)) == fused
    assert lib.sf_rollout_tok_ok(C.byref(m)) == tok


def test_is_fused_follows_process_precision(lib):
    m = rollouter(configs.C2_ROLL)
    lib.sf_set_precision(0)
    assert lib.sf_rollout_is_fused(C.byref(m)) == 0
    lib.sf_set_precision(2)   # a process default of single-pass bf16 keeps the fused layers (only the per-call modes 2 / 3 leave them)
    assert lib.sf_rollout_is_fused(C.byref(m)) == 1


@pytest.mark.parametrize('name', ['c2', 'c4', 'c5'])
def test_tok_needs_every_layer_before_the_last(lib, name):
    cfg, window = SHAPES[name]
    nl = cfg['rollout_dict']['num_layers']
    for l in range(nl - 1):
        assert lib.sf_rollout_tok_ok(C.byref(rollouter(cfg, window, null_tok_layer=l))) == 0, l
    assert lib.sf_rollout_tok_ok(C.byref(rollouter(cfg, window, null_tok_layer=nl - 1))) == 1


@pytest.mark.parametrize('name,seam', [('c2', 1), ('c5', 1), ('c4', 0), ('c4_ref', 0), ('c1', 0), ('c2_4x7', 0)])
def test_uses_seam_per_shape(lib, name, seam):
    m = rollouter(*SHAPES[name])
    assert lib.sf_rollout_uses_seam(C.byref(m), 32) == seam
    assert lib.sf_rollout_uses_seam_opts(C.byref(m), 32, None) == seam
    assert uses_seam(lib, m, 32) == seam


def test_uses_seam_only_where_a_seam_can_launch(lib):
    m = rollouter(configs.C2_ROLL)
    assert uses_seam(lib, m, 32) == 1
    assert uses_seam(lib, m, 32, precision=1) == 1
    for precision in (0, 2, 3):   # exact f32 and the single-pass modes run no fused layer
        assert uses_seam(lib, m, 32, precision=precision) == 0, precision
    assert uses_seam(lib, m, 32, attn_heads_per_wg=8) == 0
    assert uses_seam(lib, m, 32, attn_qkv_rows=128) == 0
    assert uses_seam(lib, m, 32, layer_tok=1) == 0
    assert uses_seam(lib, m, 32, seam_fused=0) == 0
    assert uses_seam(lib, m, 32, cus_available=64) == 0   # fewer CUs than the 128+ workgroups of the grid at B = 32
    assert uses_seam(lib, m, 0) == 0
    lib.sf_set_seam_fused(0)
    assert uses_seam(lib, m, 32) == 0
    assert uses_seam(lib, m, 32, seam_fused=1) == 1
    lib.sf_set_layer_tok(1)
    assert uses_seam(lib, m, 32, seam_fused=1) == 0
    assert uses_seam(lib, m, 32, seam_fused=1, layer_tok=-1) == 1


def test_uses_seam_window_of_28_tokens(lib):
    m = rollouter(configs.C2_ROLL, window=4)
    for precision in (-1, 1):
        assert uses_seam(lib, m, 32, precision=precision) == 0


@pytest.mark.parametrize('name,B,nbytes', [('c2', 1, 1330176), ('c2', 32, 42311680), ('c2', 192, 253829120), ('c4', 32, 37167104),
                                           ('c4_ref', 32, 83173376), ('c1', 32, 21733376), ('c5', 192, 284696576)])
def test_workspace_bytes(lib, name, B, nbytes):
    """One fixed layout for every plan: the same size whatever the options or process defaults."""
    m = rollouter(*SHAPES[name])
    assert lib.sf_rollout_workspace_bytes(C.byref(m), B) == nbytes
    lib.sf_set_precision(0)
    lib.sf_set_layer_tok(1)
    assert lib.sf_rollout_workspace_bytes(C.byref(m), B) == nbytes
    assert lib.sf_rollout_workspace_bytes(C.byref(m), 0) == 0
