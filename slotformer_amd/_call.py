"""What every call into libslotformer_hip needs from torch: the current stream, a raw pointer, tensors that live on the device, and a
workspace of the size the library asks for.  Imports torch alone (callers pass the library's functions in); everything else imports this."""
import torch


def stream(t=None):
    """The handle of torch's current stream on t's device (the current device when t is None)."""
    return torch.cuda.current_stream(None if t is None else t.device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def require_device(*tensors, what='inputs'):
    """Every tensor given (None is skipped) lives on a HIP device, or RuntimeError."""
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f'slotformer_amd: {what} must live on a HIP device; there is no CPU fallback')


def scratch(query, *args, device, reuse=None, empty_ok=False, at_least=0):
    """A uint8 workspace of query(*args) bytes (at least `at_least`) on `device`; query: a `*_workspace_bytes` function of the library.  `reuse`
    comes back itself when it is a buffer that large, else a fresh buffer does (nothing grows in place).  A query that returns 0 refuses the
    shape or the model without setting the library's error string, so the error is composed here; empty_ok: 0 is the size of an empty batch."""
    n = int(query(*args))
    if n == 0 and not empty_ok:
        shown = ', '.join(type(a._obj).__name__ if hasattr(a, '_obj') else repr(a) for a in args)   # (a ctypes.byref shows as its struct)
        raise RuntimeError(f'libslotformer_hip: {query.__name__}({shown}) returned 0: unsupported shape or model')
    n = max(n, at_least)
    if reuse is not None and reuse.numel() >= n:
        return reuse
    return torch.empty(n, dtype=torch.uint8, device=device)
