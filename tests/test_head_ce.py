"""CPU: what of the fused vocabulary head + cross-entropy (csrc/head_ce.hip) can be checked without a GPU -- the new symbols in header, library and
ctypes table, the shape rule at every limit, the argument errors (raised before any HIP call), the pack order of the two weight copies (the _host
twin against a NumPy restatement of the header's description), the argument checks around `fit(tokens=)`, and the split of the decoder chain."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['sf_head_ce_ok', 'sf_head_ce_packed_bytes', 'sf_head_ce_workspace_bytes', 'sf_head_ce_pack_weights', 'sf_head_ce_pack_weights_host',
       'sf_head_ce_fwd_f32', 'sf_head_ce_bwd_f32']


def lib():
    from slotformer_amd import _lib
    return _lib.lib()


def err():
    return lib().sf_last_error_string().decode()


def test_symbols_in_header_library_and_table():
    from slotformer_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'slotformer_hip.h')).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r'\b' + name + r'\s*\(([^)]*)\)', txt)
        assert decl, f'{name} is not declared in the header'
        assert hasattr(lib(), name), f'{name} is not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
        n_args = len([a for a in decl.group(1).split(',') if a.strip() and a.strip() != 'void'])
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in ('sf_head_ce_fwd_f32', 'sf_head_ce_bwd_f32', 'sf_head_ce_pack_weights'))


def test_shape_rule_at_every_limit():
    ok = lib().sf_head_ce_ok
    # K: a multiple of 32 in [32, 256]
    assert ok(4096, 32) == 1 and ok(4096, 256) == 1 and ok(4096, 192) == 1
    assert ok(4096, 0) == 0 and ok(4096, 288) == 0 and ok(4096, 48) == 0 and ok(4096, 31) == 0 and ok(4096, 33) == 0 and ok(4096, -32) == 0
    # V: a multiple of 32 in [32, 2^20]
    assert ok(32, 64) == 1 and ok(1 << 20, 64) == 1 and ok(96, 64) == 1
    assert ok(0, 64) == 0 and ok((1 << 20) + 32, 64) == 0 and ok(48, 64) == 0 and ok(31, 64) == 0 and ok(33, 64) == 0 and ok(-32, 64) == 0
    pb = lib().sf_head_ce_packed_bytes
    assert pb(4096, 192) == 4096 * 192 * 8 and pb(32, 32) == 32 * 32 * 8 and pb(4096, 288) == 0 and pb(48, 64) == 0
    wb = lib().sf_head_ce_workspace_bytes
    assert wb(1) == 16 and wb(64) == 16 and wb(65) == 32 and wb(0) == 16 and wb(-1) == 0 and wb(1 << 29) == 0 and wb((1 << 29) - 1) > 0


def test_argument_errors_without_gpu():
    """negative codes with a message, raised before any HIP call"""
    L = lib()
    one, odd, odd8 = C.c_void_p(16), C.c_void_p(20), C.c_void_p(4)
    big = 1 << 30

    def fwd(x=one, ld=64, w=one, t64=one, t16=None, gw=None, group=1, lse=one, rows=one, stats=None, R=8, V=64, K=64, ws=None, wsb=0):
        return L.sf_head_ce_fwd_f32(x, ld, w, t64, t16, gw, group, lse, rows, stats, R, V, K, ws, wsb, None)

    def bwd(x=one, ld=64, w=one, t64=one, t16=None, gw=None, group=1, lse=one, g=one, dx=one, ldx=64, R=8, V=64, K=64):
        return L.sf_head_ce_bwd_f32(x, ld, w, t64, t16, gw, group, lse, g, dx, ldx, R, V, K, None)

    for f in (fwd, bwd):
        assert f(x=None) < 0 and 'null pointer' in err()
        assert f(w=None) < 0 and 'null pointer' in err()
        assert f(lse=None) < 0 and 'null pointer' in err()
        assert f(t64=None) < 0 and 'exactly one' in err()
        assert f(t16=one) < 0 and 'exactly one' in err()
        assert f(V=100) < 0 and 'multiple of 32' in err()
        assert f(V=0) < 0 and 'multiple of 32' in err()
        assert f(K=48, ld=48) < 0 and 'multiple of 32' in err()
        assert f(K=288, ld=288) < 0 and 'multiple of 32' in err()
        assert f(t64=None, t16=one, V=32768 + 32) < 0 and 'int16' in err()
        assert f(ld=63) < 0 and 'row stride' in err()
        assert f(ld=66) < 0 and 'row stride' in err()
        assert f(R=-1) < 0 and 'row count' in err()
        assert f(R=1 << 29) < 0 and 'row count' in err()
        assert f(group=0) < 0 and 'group' in err()
        assert f(group=3) < 0 and 'group' in err()
        assert f(x=odd) < 0 and 'aligned' in err()
        assert f(w=odd) < 0 and 'aligned' in err()
    assert fwd(stats=one) < 0 and 'workspace' in err()                       # stats without a workspace
    assert fwd(stats=one, ws=one, wsb=8) < 0 and 'workspace' in err()        # ... with one too small
    assert fwd(stats=odd8, ws=one, wsb=big) < 0 and 'workspace' in err()     # ... misaligned
    assert bwd(g=None) < 0 and 'null pointer' in err()
    assert bwd(dx=None) < 0 and 'null pointer' in err()
    assert bwd(ldx=63) < 0 and 'row stride of dx' in err()
    for pack in (lambda *a: L.sf_head_ce_pack_weights(*a, None), L.sf_head_ce_pack_weights_host):
        assert pack(None, one, 64, 64) < 0 and 'null pointer' in err()
        assert pack(one, None, 64, 64) < 0 and 'null pointer' in err()
        assert pack(one, one, 48, 64) < 0 and 'multiple of 32' in err()
        assert pack(one, one, 64, 16) < 0 and 'multiple of 32' in err()


def bf16_rne(v):
    """float32 array -> its bf16 bit patterns (uint16), round to nearest even: written from the header's words, not from the library's code"""
    u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def packed_expected(w):
    """The four planes of the header's description: copy A hi | lo, copy B hi | lo."""
    V, K = w.shape
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    a = np.empty((V // 32, K // 16, 64, 8), dtype=np.float32)
    for vb in range(V // 32):
        for ks in range(K // 16):
            a[vb, ks] = w[32 * vb + (l & 31), 16 * ks + 8 * (l >> 5) + j]
    b = np.empty((V // 32, 2, K // 32, 64, 8), dtype=np.float32)
    for vb in range(V // 32):
        for c in range(2):
            for kfb in range(K // 32):
                b[vb, c, kfb] = w[32 * vb + 16 * c + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3), 32 * kfb + (l & 31)]
    planes = []
    for copy in (a, b):
        flat = copy.reshape(-1)
        hi = bf16_rne(flat)
        planes += [hi, bf16_rne(flat - bf16_value(hi))]
    return np.concatenate(planes)


@pytest.mark.parametrize('V,K', [(32, 32), (96, 64), (4096, 192), (64, 256)])
def test_pack_order_of_both_copies(V, K):
    rs = np.random.RandomState(V + K)
    w = (rs.standard_normal((V, K)) * 3).astype(np.float32)
    w[0, 0], w[V - 1, K - 1] = 0., -1e-30   # a zero and a value whose remainder underflows
    w[1, 1] = np.float32(1 + 2.**-8)        # a tie between two bf16 neighbours: rounds to the even one
    nb = lib().sf_head_ce_packed_bytes(V, K)
    assert nb == V * K * 8
    buf = np.zeros(nb // 2, dtype=np.uint16)
    assert lib().sf_head_ce_pack_weights_host(w.ctypes.data, buf.ctypes.data, V, K) == 0, err()
    want = packed_expected(w)
    assert np.array_equal(buf, want)
    # hi + lo carries the weight to 2^-16 of its size, in both copies
    n = V * K
    for c in range(2):
        back = bf16_value(buf[2 * c * n:(2 * c + 1) * n]) + bf16_value(buf[(2 * c + 1) * n:(2 * c + 2) * n])
        assert np.abs(np.sort(back) - np.sort(w.reshape(-1))).max() <= 2.**-16 * np.abs(w).max()


def test_token_table_checks():
    """`fit` / `evaluate` check tokens= before their loop: shape beside the slot table, integer dtype, device, and a model with a dVAE."""
    from slotformer_amd import video_prediction as vp
    table = SimpleNamespace(shape=(4, 12, 3, 64))
    steve = SimpleNamespace(dvae=object(), h=4, w=4)
    savi = SimpleNamespace(h=4, w=4)
    good = torch.zeros(4, 12, 16, dtype=torch.int16)
    with pytest.raises(ValueError, match='no dVAE'):
        vp._token_table(good, table, savi, 'fit')
    with pytest.raises(ValueError, match='int16 or int64'):
        vp._token_table(good.float(), table, steve, 'fit')
    with pytest.raises(ValueError, match='int16 or int64'):
        vp._token_table(good.int(), table, steve, 'fit')
    for bad in (torch.zeros(4, 11, 16, dtype=torch.int64), torch.zeros(3, 12, 16, dtype=torch.int64), torch.zeros(4, 12, 15, dtype=torch.int64),
                torch.zeros(4, 12, 4, 4, dtype=torch.int64), None):
        with pytest.raises(ValueError, match=r'\[4, 12, 16\]'):
            vp._token_table(bad, table, steve, 'evaluate')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vp._token_table(good, table, steve, 'fit')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vp._token_table(good.long(), table, steve, 'fit')
    assert 'tokens' in inspect.signature(vp.fit).parameters and 'tokens' in inspect.signature(vp.evaluate).parameters
    # the weights of the vid_len truncation: step s of clip b counts iff hist + s < clip_len[b]
    fw = vp._frame_weights(torch.tensor([[5, 3], [4, 9]], dtype=torch.int32), 3, 2)
    assert torch.equal(fw, torch.tensor([[1., 1., 0., 0.], [1., 0., 1., 1.]]))
    # the ids of the predicted frames
    tok = torch.arange(2 * 9 * 4, dtype=torch.int16).view(2, 9, 4)
    ids = vp._clip_token_ids(tok, torch.tensor([1, 0], dtype=torch.int32), torch.tensor([2, 0], dtype=torch.int32), 2, 2, 2)
    assert ids.dtype == torch.int16 and torch.equal(ids, torch.stack([tok[1, 6], tok[1, 8], tok[0, 4], tok[0, 6]]))


def test_no_cpu_fallback_and_frozen_head_only():
    from slotformer_amd import ops, train
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pack_head_ce_weight(torch.zeros(64, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.head_ce_forward(torch.zeros(4, 64), torch.zeros(64 * 64 * 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.head_cross_entropy(torch.zeros(4, 64), torch.zeros(64, 64), torch.zeros(4, dtype=torch.int64))


def test_decoder_chain_is_split_at_the_head():
    from slotformer_amd import train
    assert callable(train.slate_decoder_hidden) and callable(train.head_cross_entropy)
    src = inspect.getsource(train.slate_decoder_forward)
    assert 'slate_decoder_hidden(dec, slots, idx)' in src and 'dec.head' in src
    assert 'dec.head' not in inspect.getsource(train.slate_decoder_hidden)
