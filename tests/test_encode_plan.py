"""CPU: the encode's plan as the C ABI reports it (sf_savi_chain_ok and the workspace queries of sf_savi_encode_*, sf_savi_cnn_f32,
sf_savi_features_planes_f32 and sf_savi_slots_chain_f32) for the encoders of configs.py.  The encoders carry dummy non-null weight pointers: the plan
reads which weights and packed copies are there, never a weight.  tests/golden/encode_ws_bytes.json holds what every query returns per config, process
precision, batch and clip length."""
import ctypes as C
import json
import os

import pytest

from slotformer_amd import configs

DUMMY = 0x1000   # never dereferenced
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encode_ws_bytes.json')
NOT_SET = ('pred_layers', 'pred_packed')   # read by the encode itself, not by its plan
PROLOGUE_PACKED = ('pm_w0_p', 'pm_w2_p', 'kd_w0_p')


def encoder(cfg, prologue_packed=True):
    """sf_savi_encoder of a savi_cfg(): the shape of engine.py's, every other weight pointer DUMMY (prologue_packed=False: without the packed
    predictor / kernel_dist copies the NEXT-step prologue and the slot chain need)"""
    from slotformer_amd import _lib
    m = _lib.sf_savi_encoder()
    for f, t in _lib.sf_savi_encoder._fields_:
        if t is _lib.FP or t is C.c_void_p:
            setattr(m, f, None if f in NOT_SET or (f in PROLOGUE_PACKED and not prologue_packed) else DUMMY)
    ed, sd, pd = cfg['enc_dict'], cfg['slot_dict'], cfg['pred_dict']
    ch = ed['enc_channels']
    m.resolution, m.enc_layers, m.enc_ks = cfg['resolution'][0], len(ch) - 1, ed['enc_ks']
    for i, c in enumerate(ch):
        m.enc_channels[i] = c
    for i in range(len(ch) - 1):
        m.conv_w[i] = m.conv_b[i] = DUMMY
        m.conv_w_frag[i] = DUMMY if i > 0 else None
    m.enc_out_channels = ed['enc_out_channels']
    m.num_slots, m.slot_size, m.slot_mlp_size, m.num_iterations = sd['num_slots'], sd['slot_size'], sd['slot_mlp_size'], sd['num_iterations']
    m.sa_eps = 1e-6
    stochastic = cfg['model'] != 'STEVE'   # STEVE has no kernel distribution
    m.kd_mode = (2 if sd['kernel_mlp'] else 1) if stochastic else 0
    mlp = pd['pred_type'] == 'mlp'
    m.pred_type, m.pred_rnn, m.pred_norm_first = 0 if mlp else 1, int(pd['pred_rnn']), int(pd['pred_norm_first'])
    m.pred_num_layers, m.pred_num_heads = pd['pred_num_layers'], pd['pred_num_heads']
    m.pred_ffn_dim = 2 * sd['slot_size'] if mlp else pd['pred_ffn_dim']
    m.pred_hidden = sd['slot_mlp_size'] if pd['pred_rnn'] else 0
    return m


ENCODERS = {
    'c1': (configs.C1_SAVI, True),        # 64 x 64, Transformer + LSTM predictor, kernel MLP
    'c2': (configs.C2_SAVI, True),        # 128 x 128, residual-MLP predictor, one-Linear kernel_dist: the slot chain applies
    'c2_unpacked': (configs.C2_SAVI, False),   # ... without the packed prologue copies: no NEXT-step prologue, no slot chain
    'c4': (configs.C4_STEVE, True),       # slot size 192, no kernel distribution
    'c5': (configs.C5_SAVI, True),        # 8 slots
    'train': (configs.TRAIN_SAVI, True),  # C2's slot branch at 64 x 64
}
BATCHES = (1, 5, 32, 33)        # 33: more than one CNN chunk, no batched form
CLIPS = (1, 2, 6, 13)           # 32 x 13 = 416 frames: over the batched form's 384


def record(lib, m, B, T):
    """every query the golden file pins, for one encoder, batch and clip length under the current process precision"""
    mp = C.byref(m)
    r = {
        'encode': lib.sf_savi_encode_workspace_bytes(mp, B),
        'fork': lib.sf_savi_encode_fork_workspace_bytes(mp, B, T),
        'cnn': lib.sf_savi_cnn_workspace_bytes(mp, B),
        'features': lib.sf_savi_features_workspace_bytes(mp, B, T),
        'slots_chain': lib.sf_savi_slots_chain_workspace_bytes(mp, B),
        'planes': lib.sf_savi_planes_bytes(mp, B, T),
        'chain_ok': lib.sf_savi_chain_ok(mp, B, T),
    }
    for chain in (0, 1):
        lib.sf_set_slot_chain(chain)
        r['batched_chain%d' % chain] = lib.sf_savi_encode_batched_workspace_bytes(mp, B, T)
    lib.sf_set_slot_chain(0)
    return r


@pytest.fixture
def lib():
    """Process defaults the plan depends on: split-bf16, slot chain off, bf16 attention planes on, NEXT-step prologue on -- restored afterwards."""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision(), lib.sf_get_slot_chain(), lib.sf_get_slot_attn_planes(), lib.sf_get_encode_fuse_next()
    lib.sf_set_precision(1)
    lib.sf_set_slot_chain(0)
    lib.sf_set_slot_attn_planes(1)
    lib.sf_set_encode_fuse_next(1)
    yield lib
    lib.sf_set_precision(old[0])
    lib.sf_set_slot_chain(old[1])
    lib.sf_set_slot_attn_planes(old[2])
    lib.sf_set_encode_fuse_next(old[3])


@pytest.mark.parametrize('precision', [1, 0])
@pytest.mark.parametrize('name', list(ENCODERS))
def test_workspace_bytes(lib, name, precision):
    with open(GOLDEN) as f:
        golden = json.load(f)
    m = encoder(*ENCODERS[name])
    lib.sf_set_precision(precision)
    for B in BATCHES:
        for T in CLIPS:
            key = '%s/p%d/B%d/T%d' % (name, precision, B, T)
            assert record(lib, m, B, T) == golden[key], key


@pytest.mark.parametrize('name,ok', [('c2', 1), ('train', 1), ('c2_unpacked', 0), ('c1', 0), ('c4', 0), ('c5', 0)])
def test_chain_ok_per_shape(lib, name, ok):
    m = encoder(*ENCODERS[name])
    assert lib.sf_savi_chain_ok(C.byref(m), 32, 6) == ok
    assert lib.sf_savi_chain_ok(C.byref(m), 32, 13) == 0   # 416 frames
    assert lib.sf_savi_chain_ok(C.byref(m), 32, 1) == 0
    assert lib.sf_savi_chain_ok(C.byref(m), 33, 6) == 0
    lib.sf_set_precision(0)
    assert lib.sf_savi_chain_ok(C.byref(m), 32, 6) == 0
    lib.sf_set_precision(1)
    lib.sf_set_encode_fuse_next(0)
    assert lib.sf_savi_chain_ok(C.byref(m), 32, 6) == 0


def test_batched_workspace_holds_the_chain_planes_only_for_the_chain(lib):
    """C2 at B = 32, T = 6: the slot-chain feature planes (402,653,184 bytes) only under sf_set_slot_chain(1)"""
    m = encoder(configs.C2_SAVI)
    base = lib.sf_savi_encode_workspace_bytes(C.byref(m), 32)
    batched = lib.sf_savi_encode_batched_workspace_bytes(C.byref(m), 32, 6)
    assert batched - base == 3 * 32 * 6 * 4096 * 64 * 4   # the activations of the 192 frames
    lib.sf_set_slot_chain(1)
    assert lib.sf_savi_encode_batched_workspace_bytes(C.byref(m), 32, 6) - batched == 402653184 == lib.sf_savi_planes_bytes(C.byref(m), 32, 6)
    m = encoder(configs.C2_SAVI, prologue_packed=False)   # no chain for this model: no planes
    assert lib.sf_savi_encode_batched_workspace_bytes(C.byref(m), 32, 6) == batched
