"""CPU: slotformer_amd._call, the one home of the plumbing around a library call -- the workspace of the size a `*_workspace_bytes` query returns
(and the error, composed in Python, for a query that returns 0), the raw pointer and the residency check.  The queries are host arithmetic, so
the built library is all this needs; the buffers live on the CPU device, which is enough for the helper's logic."""
import ctypes as C

import pytest
import torch

from slotformer_amd import _call, _lib

CPU = torch.device('cpu')


@pytest.fixture()
def lib():
    return _lib.lib()


@pytest.mark.parametrize('query, args', [('sf_physion_readout_bwd_workspace_bytes', (0, 7, 64)),       # no batch
                                         ('sf_aloe_workspace_bytes', (2, 4, 3, 5, 6, 64))])             # d_model 6: no multiple of 4
def test_zero_query_names_itself_and_not_the_last_library_error(lib, query, args):
    assert lib.sf_set_precision(3) < 0 and b'precision' in lib.sf_last_error_string()   # an unrelated failure, left in the error string
    with pytest.raises(RuntimeError) as e:
        _call.scratch(getattr(lib, query), *args, device=CPU)
    msg = str(e.value)
    assert query in msg and ', '.join(map(str, args)) in msg and 'returned 0' in msg
    assert 'precision' not in msg


def test_zero_query_shows_a_struct_argument_by_its_type(lib):
    with pytest.raises(RuntimeError, match=r'sf_rollout_workspace_bytes\(sf_rollouter, 0\) returned 0'):
        _call.scratch(lib.sf_rollout_workspace_bytes, C.byref(_lib.sf_rollouter()), 0, device=CPU)


def test_size_is_the_query_or_the_floor(lib):
    need = lib.sf_physion_readout_bwd_workspace_bytes(2, 4, 64)
    assert need == 2 * 64 * (1 + 2 * 4) * 4
    ws = _call.scratch(lib.sf_physion_readout_bwd_workspace_bytes, 2, 4, 64, device=CPU)
    assert ws.dtype == torch.uint8 and ws.device == CPU and ws.numel() == need
    assert _call.scratch(lib.sf_physion_readout_bwd_workspace_bytes, 2, 4, 64, device=CPU, at_least=16).numel() == need
    assert lib.sf_kv_producer_workspace_bytes(1, 1) == 8
    assert _call.scratch(lib.sf_kv_producer_workspace_bytes, 1, 1, device=CPU, at_least=16).numel() == 16


def test_reuse_returns_the_buffer_or_a_fresh_one(lib):
    q, args = lib.sf_physion_readout_bwd_workspace_bytes, (2, 4, 64)
    need = q(*args)
    for big in (torch.empty(need, dtype=torch.uint8), torch.empty(need + 100, dtype=torch.uint8)):
        assert _call.scratch(q, *args, device=CPU, reuse=big) is big
    small = torch.empty(need - 1, dtype=torch.uint8)
    ws = _call.scratch(q, *args, device=CPU, reuse=small)
    assert ws is not small and ws.numel() == need and small.numel() == need - 1   # replaced, not grown in place
    assert _call.scratch(q, *args, device=CPU, reuse=None).numel() == need
    with pytest.raises(RuntimeError, match='returned 0'):                         # a buffer to reuse does not excuse an unsupported shape
        _call.scratch(q, 0, 7, 64, device=CPU, reuse=big)


def test_empty_batch_is_a_size_only_where_the_site_says_so(lib):
    assert lib.sf_groupnorm1_workspace_bytes(0) == 0
    ws = _call.scratch(lib.sf_groupnorm1_workspace_bytes, 0, device=CPU, empty_ok=True, at_least=8)
    assert ws.dtype == torch.uint8 and ws.numel() == 8
    with pytest.raises(RuntimeError, match=r'sf_groupnorm1_workspace_bytes\(0\) returned 0'):
        _call.scratch(lib.sf_groupnorm1_workspace_bytes, 0, device=CPU, at_least=8)


def test_ptr_and_require_device():
    assert _call.ptr(None) is None
    t = torch.zeros(3)
    assert _call.ptr(t) == t.data_ptr()
    _call.require_device(None)
    _call.require_device()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _call.require_device(None, t)
    with pytest.raises(RuntimeError, match='slotformer_amd: the slot table must live on a HIP device; there is no CPU fallback'):
        _call.require_device(t, what='the slot table')
    with pytest.raises(RuntimeError, match='inputs must live on a HIP device'):
        _call.require_device([1, 2])   # not a tensor at all
