"""CPU: which rollouts take token-stationary layer launches, as sf_rollout_tok_layers reports it -- the OBJ3D Transformer (configs.C1_ROLL: d_model 128,
8 heads of 16, ffn 512; generic path + csrc/layer_tok128.hip) and the d_model 256 rollouters (fused / long-window paths + csrc/layer_tok.hip).
Dummy non-null weight pointers as in test_rollout_plan.py: the plan reads which packed copies are there, never a weight."""
import ctypes as C

import pytest

from slotformer_amd import configs

DUMMY = 0x1000   # never dereferenced


def rollouter(cfg, window=None, null_tok_layers=(), norm_first=None):
    from slotformer_amd import _lib
    rd = cfg['rollout_dict']
    nl = rd['num_layers']
    layers = (_lib.sf_tfm_layer * nl)()
    for i, layer in enumerate(layers):
        for f, _ in _lib.sf_tfm_layer._fields_:
            setattr(layer, f, None if (f == 'tok_packed' and i in null_tok_layers) else DUMMY)
    single = 'cond_len' in rd
    W = window or (rd['cond_len'] if single else rd['history_len'])
    nf = int(rd['norm_first']) if norm_first is None else norm_first
    m = _lib.sf_rollouter(rd['num_slots'], rd['slot_size'], rd['d_model'], nl, rd['num_heads'], rd['ffn_dim'], nf, W, int(single))
    for f in ('in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'pe_tok', 'in_proj_packed', 'out_proj_packed'):
        setattr(m, f, DUMMY)
    m.layers = C.cast(layers, C.POINTER(_lib.sf_tfm_layer))
    m._layers = layers   # keeps the array alive
    return m


@pytest.fixture
def lib():
    """Process defaults the plan depends on: split-bf16, token-stationary layers off -- restored afterwards."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision(), lib.sf_get_layer_tok()
    lib.sf_set_precision(1)
    lib.sf_set_layer_tok(0)
    yield lib
    lib.sf_set_precision(old[0])
    lib.sf_set_layer_tok(old[1])


def opts(**kw):
    from slotformer_amd import _lib
    o = dict(precision=-1, seam_fused=-1, ffn_rows=0, attn_heads_per_wg=0, attn_qkv_rows=0, ffn_tile=0, cus_available=0, layer_tok=0)
    o.update(kw)
    return _lib.sf_rollout_opts(**o)


def tok_layers(lib, m, B=32, **kw):
    return lib.sf_rollout_tok_layers(C.byref(m), B, C.byref(opts(**kw)))


def stays_generic(lib, m):
    return lib.sf_rollout_tok_ok(C.byref(m)) == 0 and lib.sf_rollout_is_fused(C.byref(m)) == 0


def test_obj3d_shape():
    rd = configs.C1_ROLL['rollout_dict']
    assert (rd['d_model'], rd['num_heads'], rd['ffn_dim'], rd['num_layers'], rd['num_slots'] * rd['history_len']) == (128, 8, 512, 4, 36)


def test_obj3d_follows_the_option_and_the_process_default(lib):
    m = rollouter(configs.C1_ROLL)
    assert tok_layers(lib, m, layer_tok=1) == 3
    assert tok_layers(lib, m, layer_tok=-1) == 0
    assert tok_layers(lib, m, layer_tok=0) == 0                        # the process default is OFF
    assert lib.sf_rollout_tok_layers(C.byref(m), 32, None) == 0
    assert stays_generic(lib, m)
    lib.sf_set_layer_tok(1)
    assert tok_layers(lib, m, layer_tok=0) == 3
    assert lib.sf_rollout_tok_layers(C.byref(m), 32, None) == 3
    assert tok_layers(lib, m, layer_tok=-1) == 0
    assert stays_generic(lib, m)                                       # sf_rollout_tok_ok answers for the FUSED-layer path only
    for B in (1, 3, 192, 512):
        assert tok_layers(lib, m, B=B, layer_tok=1) == 3, B
    assert tok_layers(lib, m, B=0, layer_tok=1) == 0


def test_obj3d_precision_gate(lib):
    m = rollouter(configs.C1_ROLL)
    assert tok_layers(lib, m, layer_tok=1, precision=1) == 3
    for precision in (0, 2, 3):   # exact f32 and the per-call single-pass modes run every product on the GEMM core
        assert tok_layers(lib, m, layer_tok=1, precision=precision) == 0, precision
    lib.sf_set_precision(0)
    assert tok_layers(lib, m, layer_tok=1) == 0
    assert tok_layers(lib, m, layer_tok=1, precision=1) == 3
    assert stays_generic(lib, m)


def test_obj3d_needs_every_layer_before_the_last(lib):
    for l in range(3):
        m = rollouter(configs.C1_ROLL, null_tok_layers=(l, ))
        assert tok_layers(lib, m, layer_tok=1) == 0, l
        assert stays_generic(lib, m)
    assert tok_layers(lib, rollouter(configs.C1_ROLL, null_tok_layers=(3, )), layer_tok=1) == 3


def test_obj3d_norm_first_and_window(lib):
    assert tok_layers(lib, rollouter(configs.C1_ROLL, norm_first=0), layer_tok=1) == 0
    long = rollouter(configs.C1_ROLL, window=17)    # 17 frames x 6 slots = 102 tokens: past the kernel's 96
    assert tok_layers(lib, long, layer_tok=1) == 0
    assert stays_generic(lib, long)
    assert tok_layers(lib, rollouter(configs.C1_ROLL, window=16), layer_tok=1) == 3   # 96 tokens: one video per workgroup
    assert tok_layers(lib, rollouter(configs.C1_ROLL, window=1), layer_tok=1) == 3


def test_obj3d_workspace_is_the_same_with_the_option_on_and_off(lib):
    m = rollouter(configs.C1_ROLL)
    off = lib.sf_rollout_workspace_bytes(C.byref(m), 32)
    lib.sf_set_layer_tok(1)
    assert lib.sf_rollout_workspace_bytes(C.byref(m), 32) == off == 21733376


# (config, sf_rollout_tok_ok): C4_ROLL_REF is the long-window path (90 tokens) -- not the fused-layer path, yet its seven leading layers are taken
@pytest.mark.parametrize('name,tok_ok', [('C2_ROLL', 1), ('C4_ROLL', 1), ('C4_ROLL_REF', 0), ('C5_ROLL', 1)])
def test_d256_shapes_report_the_layers_they_take_today(lib, name, tok_ok):
    cfg = getattr(configs, name)
    m = rollouter(cfg)
    nl = cfg['rollout_dict']['num_layers']
    assert lib.sf_rollout_tok_ok(C.byref(m)) == tok_ok
    assert tok_layers(lib, m, layer_tok=1) == nl - 1
    assert tok_layers(lib, m, layer_tok=-1) == 0
    assert tok_layers(lib, m, layer_tok=0) == 0
    assert tok_layers(lib, m, layer_tok=1, precision=0) == 0
    assert tok_layers(lib, rollouter(cfg, null_tok_layers=(0, )), layer_tok=1) == 0


def test_packed_bytes_per_shape(lib):
    big = lib.sf_layer_tok_packed_bytes()
    assert lib.sf_layer_tok_packed_bytes_ex(256, 8, 1024) == big == 96 * 32768 + 3328 * 4
    small = lib.sf_layer_tok_packed_bytes_ex(128, 8, 512)
    assert small == 48 * 16384 + 1664 * 4     # 196,608 weight elements as hi | lo bf16 + the layer's eight vectors
    for shape in ((128, 4, 512), (64, 8, 256), (256, 8, 512), (128, 8, 1024), (0, 0, 0)):
        assert lib.sf_layer_tok_packed_bytes_ex(*shape) == 0, shape
