"""CPU: what of the head's weight gradient (sf_head_ce_wgrad_f32 in csrc/head_ce.hip, `head_cross_entropy(..., weight_grad=True)`,
`STEVE.fused_token_loss`) can be checked without a GPU -- the two symbols in header, library and ctypes table, the workspace rule at every
limit and its independence of R, every argument error (raised before any HIP call), the missing CPU fallback and the attribute's default."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['sf_head_ce_wgrad_workspace_bytes', 'sf_head_ce_wgrad_f32']


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
    assert all(name in doc for name in NEW) and 'fused_token_loss' in doc and 'weight_grad' in doc


def test_workspace_rule():
    wb = lib().sf_head_ce_wgrad_workspace_bytes
    assert wb(1, 32, 32) == 32 * 32 * 4                       # one tile: one split
    assert wb(73728, 4096, 192) > 0 and wb((1 << 29) - 1, 4096, 192) > 0
    assert wb(73728, 4096, 48) == 0 and wb(73728, 4096, 288) == 0 and wb(73728, 48, 64) == 0
    assert wb(-1, 4096, 192) == 0 and wb(1 << 29, 4096, 192) == 0
    # whole [V, K] blocks, at most eight of them, and no more of them for more rows
    for V, K in ((4096, 192), (64, 64), (1 << 20, 256)):
        block = V * K * 4
        sizes = [wb(R, V, K) for R in (1, 32, 33, 256, 257, 8192, 73728, 2 * 73728, (1 << 29) - 1)]
        assert all(s % block == 0 and 1 <= s // block <= 8 for s in sizes), (V, K, sizes)
        assert sizes[0] == block
        assert wb(73728, V, K) == wb(2 * 73728, V, K) == wb((1 << 29) - 32, V, K)
    assert wb(73728, 4096, 192) == 8 * 4096 * 192 * 4         # 32 slabs of 128 words: eight splits fill 256 workgroups
    assert wb(73728, 1 << 20, 256) == (1 << 20) * 256 * 4     # 8192 slabs need no split


def test_argument_errors_without_gpu():
    """negative codes with a message, raised before any HIP call"""
    L = lib()
    one, odd = C.c_void_p(16), C.c_void_p(20)
    big = 1 << 40

    def wg(x=one, ld=64, w=one, t64=one, t16=None, gw=None, lse=one, g=one, dW=one, ldw=64, R=8, V=64, K=64, group=1, ws=one, wsb=big):
        return L.sf_head_ce_wgrad_f32(x, ld, w, t64, t16, gw, lse, g, dW, ldw, R, V, K, group, ws, wsb, None)

    for name in ('x', 'w', 'lse', 'g', 'dW', 'ws'):
        assert wg(**{name: None}) < 0 and 'null pointer' in err(), name
    assert wg(t64=None) < 0 and 'exactly one' in err()
    assert wg(t16=one) < 0 and 'exactly one' in err()
    assert wg(V=100) < 0 and 'multiple of 32' in err()
    assert wg(V=0) < 0 and 'multiple of 32' in err()
    assert wg(K=48, ld=48, ldw=48) < 0 and 'multiple of 32' in err()
    assert wg(K=288, ld=288, ldw=288) < 0 and 'multiple of 32' in err()
    assert wg(t64=None, t16=one, V=32768 + 32) < 0 and 'int16' in err()
    assert wg(ld=63) < 0 and 'row stride of x' in err()
    assert wg(ld=66) < 0 and 'row stride of x' in err()
    assert wg(ldw=63) < 0 and 'row stride of dW' in err()
    assert wg(R=-1) < 0 and 'row count' in err()
    assert wg(R=1 << 29) < 0 and 'row count' in err()
    assert wg(group=0) < 0 and 'group' in err()
    assert wg(group=3) < 0 and 'group' in err()
    assert wg(x=odd) < 0 and 'aligned' in err()
    assert wg(w=odd) < 0 and 'aligned' in err()
    assert wg(ws=odd) < 0 and 'workspace' in err()
    assert wg(wsb=64 * 64 * 4 - 1) < 0 and 'workspace' in err()
    assert wg(R=64, wsb=64 * 64 * 4) < 0 and 'workspace' in err()   # two tiles: two splits of a one-slab head


def test_no_cpu_fallback():
    from slotformer_amd import ops, train
    w = torch.zeros(64, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        train.head_cross_entropy(torch.zeros(4, 64), w, torch.zeros(4, dtype=torch.int64), weight_grad=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.head_ce_wgrad(torch.zeros(4, 64), torch.zeros(64 * 64 * 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), 64, torch.zeros(4),
                          torch.ones(1))


def test_steve_attribute_defaults_to_off():
    from slotformer_amd.base_slots.models.steve import STEVE
    assert STEVE.fused_token_loss is False
    import golden_util as gu
    from slotformer_amd.base_slots import build_model
    m = build_model(gu.ParamsView(gu.steve_tokens_cfg()))
    assert m.fused_token_loss is False
    m.fused_token_loss = True
    assert STEVE.fused_token_loss is False   # set on the model, not on the class
