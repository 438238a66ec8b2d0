"""CPU: the plan cache (slotformer_amd/plans.py) -- one signature, one cache attribute per owner that copies and pickles as empty, one
`invalidate` -- and the modules that keep their derived weight copies in it."""
import copy
import ctypes as C
import io

import torch
from torch import nn

from slotformer_amd import engine, plans


class _Desc(C.Structure):
    _fields_ = [('w', C.c_void_p), ('rows', C.POINTER(C.c_void_p))]


class _Owner(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(4, 3)
        self.register_buffer('table', torch.arange(6.))


def _roundtrip(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _decoder():
    from slotformer_amd.base_slots.models.steve_transformer import STEVETransformerDecoder
    return STEVETransformerDecoder(64, 32, 4, 16, 3, 2).eval()


def test_cached_hit_rebuild_and_names():
    m, built = _Owner(), []

    def build(tag):
        built.append(tag)
        return [tag, len(built)]
    get = lambda name: plans.cached(m, name, plans.signature(m), build, name)  # noqa: E731
    a = get('a')
    assert get('a') is a and built == ['a']                       # a hit: the same object, nothing built
    b = get('b')
    assert b is not a and get('b') is b and get('a') is a         # a second name on the same owner is independent
    with torch.no_grad():
        m.lin.weight.add_(0)                                      # a version bump
    a2 = get('a')
    assert a2 is not a and a2 == ['a', 3] and get('a') is a2
    plans.invalidate(m)
    a3 = get('a')
    assert a3 is not a2 and get('a') is a3
    # no growth: one entry per name, the old value gone
    store = m.__dict__[plans._ATTR]
    assert set(store) == {'a'} and not any(a2 is x for entry in store.values() for x in entry)
    b2 = get('b')
    assert b2 is not b and set(store) == {'a', 'b'} and len([k for k in m.__dict__ if 'plan' in k]) == 1


def test_plan_receives_the_signature_and_keeps_what_dp_returns():
    m = _Owner()

    def build():
        plan = plans.Plan()
        plan.struct = _Desc(w=plan.dp(m.lin.weight), rows=None)
        assert plan.dp(None) is None
        return plan
    plan = plans.cached(m, 'p', plans.signature(m), build)
    assert plan.sig == plans.signature(m) and plan.struct.w == m.lin.weight.data_ptr() and plan.keep[0].data_ptr() == plan.struct.w
    half = m.lin.weight.detach().double()                          # not float32: dp() converts and keeps the copy
    assert plan.dp(half) == plan.keep[-1].data_ptr() != half.data_ptr() and plan.keep[-1].dtype == torch.float32


def test_signature_covers_buffers_and_bare_tensors():
    m = _Owner()
    want = tuple((t.data_ptr(), t._version) for t in (m.lin.weight, m.lin.bias, m.table))
    assert plans.signature(m) == want
    assert plans.signature(m.lin.bias, m.lin) == (want[1], want[0], want[1])     # in the order given
    m.table.add_(0)
    after = plans.signature(m)
    assert after[:2] == want[:2] and after[2] != want[2]


def test_ctypes_pointers_in_the_cache_survive_deepcopy_and_pickling():
    m = _Owner()

    def build():
        rows = (C.c_void_p * 2)(m.lin.weight.data_ptr(), m.lin.bias.data_ptr())
        return _Desc(w=m.lin.weight.data_ptr(), rows=C.cast(rows, C.POINTER(C.c_void_p))), rows
    held = plans.cached(m, 'desc', plans.signature(m), build)
    for other in (copy.deepcopy(m), _roundtrip(m)):
        assert torch.equal(other.lin.weight, m.lin.weight)
        assert not other.__dict__.get(plans._ATTR)                 # the copy starts with an empty cache
        seen = []
        plans.cached(other, 'desc', plans.signature(other), lambda: seen.append(1) or 'rebuilt')
        assert seen == [1]
    assert plans.cached(m, 'desc', plans.signature(m), build) is held   # the original keeps its own


def test_slate_plan_is_copied_and_pickled_as_the_copy_s_own():
    """Fails on the parent commit: the slate plan was a tuple holding a ctypes structure, and `copy.deepcopy` / `torch.save` of a decoder that
    had built it raised `ValueError: ctypes objects containing pointers cannot be pickled`."""
    dec = _decoder()
    plan = dec._slate_plan()
    assert dec._slate_plan() is plan and plan.struct.head_w == dec.head.weight.data_ptr()
    for other in (copy.deepcopy(dec), _roundtrip(dec)):
        mine = other._slate_plan()
        assert mine is not plan and mine.struct.head_w == other.head.weight.data_ptr() != dec.head.weight.data_ptr()
        assert mine.struct.tok_emb == other.tok_emb.weight.data_ptr() and mine.struct.num_layers == 2
    assert dec._slate_plan() is plan
    with torch.no_grad():
        dec.pos_emb.pe.add_(0)                                      # the position table the plan reads
    assert dec._slate_plan() is not plan


def test_catw_after_invalidate():
    """Fails on the parent commit: `invalidate` deleted `_cat`, which only `__init__` created, and the next `_catw` raised AttributeError."""
    dec = _decoder()
    sa = dec.tf_dec.blocks[0].self_attn
    ws = (sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight)
    a = dec._catw('sa0', *ws)
    assert dec._catw('sa0', *ws) is a and torch.equal(a, torch.cat([w.detach() for w in ws], 0))
    dec._slate_plan()
    engine.invalidate(dec)
    b = dec._catw('sa0', *ws)
    assert b is not a and torch.equal(b, a) and dec._catw('sa0', *ws) is b
    with torch.no_grad():
        sa.proj_k.weight.mul_(2.)
    c = dec._catw('sa0', *ws)
    assert c is not b and torch.equal(c, torch.cat([w.detach() for w in ws], 0)) and not torch.equal(c, b)


def test_rollouter_plan_identity_on_the_cpu():
    from slotformer_amd.video_prediction.models import SlotRollouter
    r = SlotRollouter(num_slots=3, slot_size=16, history_len=2, d_model=32, num_layers=1, num_heads=2, ffn_dim=64).eval()
    plan = engine.rollouter_plan(r, packed=False)
    assert engine.rollouter_plan(r, packed=False) is plan                      # the same object while nothing changed
    assert plan.sig == plans.signature(r) and plan.struct.in_proj_w == r.in_proj.weight.data_ptr()
    assert (plan.struct.d_model, plan.struct.num_layers, plan.struct.window_len) == (32, 1, 2) and not plan.struct.in_proj_packed
    with torch.no_grad():
        r.out_proj.bias.add_(0)
    bumped = engine.rollouter_plan(r, packed=False)
    assert bumped is not plan and engine.rollouter_plan(r, packed=False) is bumped   # a new one after a version bump ...
    engine.invalidate(r)
    assert engine.rollouter_plan(r, packed=False) is not bumped                      # ... and after invalidate
    r2 = copy.deepcopy(r)
    assert engine.rollouter_plan(r2, packed=False).struct.in_proj_w == r2.in_proj.weight.data_ptr() != r.in_proj.weight.data_ptr()


def test_no_module_creates_a_cache_in_its_constructor():
    from slotformer_amd.base_slots.models.dVAE import dVAE
    from slotformer_amd.lpips import LPIPS
    for m in (dVAE(64), _decoder(), LPIPS()):
        for sub in m.modules():
            assert not {'_packed', '_cat', '_plan', '_sf_plan', '_sf_plans'} & set(sub.__dict__), type(sub).__name__
