"""The one cache for the derived copies of weights the host code keeps: ctypes descriptors, fragment-ordered split-bf16 buffers,
concatenated and transposed matrices.  A copy is valid while the `signature` of what it was derived from stands: (data_ptr, _version) of
the tensors, which follows optimizer steps and ordinary in-place ops.  Writes that bypass torch's version counter (`p.data.copy_()`,
raw-pointer kernels) need `invalidate(module)` -- or `torch._C._increment_version(p)`.

Every cache of an owner lives in one instance attribute, created on demand, that deep-copies and pickles as empty: a copied module
rebuilds its plans from its own tensors, whatever the plans hold (ctypes structures with raw pointers included)."""
import torch

_ATTR = '_sf_plans'


def signature(*things):
    """(data_ptr, _version) of the parameters and buffers of modules and of bare tensors, in the order given."""
    ts = []
    for x in things:
        if isinstance(x, torch.nn.Module):
            ts += x.parameters()
            ts += x.buffers()
        else:
            ts.append(x)
    return tuple((t.data_ptr(), t._version) for t in ts)


class Plan:
    """ctypes descriptor + the tensors it points to."""

    def __init__(self):
        self.keep = []
        self.struct = None
        self.sig = None

    # a plan held outside the cache (a pipeline keeps the one its graphs point into) copies / pickles as a fresh one, like the cache
    def __deepcopy__(self, memo):
        return Plan()

    def __reduce__(self):
        return (Plan, ())

    def f32(self, t):
        """`t` as a detached contiguous float32 tensor the plan keeps alive."""
        t = t.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.float().contiguous()
        self.keep.append(t)
        return t

    def dp(self, t):
        return None if t is None else self.f32(t).data_ptr()

    def packed(self, w):
        """Device pointer of the fragment-ordered split-bf16 copy of the torch-layout matrix `w` (`ops.pack_linear`), kept alive."""
        from . import ops
        self.keep.append(ops.pack_linear(self.f32(w)))
        return self.keep[-1].data_ptr()


class _Plans(dict):
    """name -> (signature, value) of one owner."""

    def __deepcopy__(self, memo):
        return _Plans()

    def __reduce__(self):
        return (_Plans, ())


def cached(owner, name, sig, build, *args):
    """The value cached on `owner` under `name` while `sig` stands, else `build(*args)`, which replaces it (a Plan receives `sig`)."""
    plans = owner.__dict__.get(_ATTR)
    if plans is None:
        plans = owner.__dict__[_ATTR] = _Plans()
    hit = plans.get(name)
    if hit is not None and hit[0] == sig:
        return hit[1]
    value = build(*args)
    if isinstance(value, Plan):
        value.sig = sig
    plans[name] = (sig, value)
    return value


def invalidate(module):
    """Drop every cached plan (packed / derived weight copies) below `module`."""
    for m in module.modules():
        m.__dict__.pop(_ATTR, None)
