"""The host side of one native call, once: dtype code, pointer, raw stream, device guard, device check — and `launch`, the
call every device entry of the C ABI fits (include/*.h: the stream is the last argument, truthy means success)."""
import torch

from . import _lib
from ._lib import CSPN_F16, CSPN_F32


def _dt(t):
    if t.dtype == torch.float32:
        return CSPN_F32
    if t.dtype == torch.float16:
        return CSPN_F16
    raise TypeError("CSPN HIP engine supports float32 / float16 tensors, got %s" % t.dtype)


def _require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("CSPN HIP engine: tensors must live on a ROCm device (got %s); "
                               "there is no CPU implementation in this package" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("CSPN HIP engine: tensors on different devices (%s vs %s)" % (dev, t.device))
    return dev


class _device_guard(object):
    """`with torch.cuda.device(dev)` only when `dev` is not already current (the common case costs ~nothing)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index)       # (a plain int: the argtypes say c_void_p; no Stream object per call)


def _p(t):
    return None if t is None else t.data_ptr()                  # (a plain int, as above: ~0.4 us per argument less than a c_void_p object)


def launch(dev, name, *args):
    """The entry `name` on `dev`'s current stream, enqueued with `dev` current; raises with the library's message if it refuses."""
    with _device_guard(dev):
        ok = getattr(_lib.lib(), name)(*args, _stream(dev))
    _lib.check(ok, name)
