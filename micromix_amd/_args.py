"""What every wrapper of the C ABI does around its launch: check the tensors, allocate or check the outputs, find the entry, launch
on torch's current stream and turn the status into an exception.  Private to the package; mixedgemm.py, paged.py and moe_ops.py are
built on it.

The rule of the hot path: the cheap test inline, the helper that words the error only once that test failed.  A successful call pays
for one short-circuit expression per tensor and makes no torch call beyond the allocations the wrapper documents."""
from __future__ import annotations

import torch

from . import _lib


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_tensor(t, name, dtype, device=None):
    """Slow path: produces the precise error.  The ops call it only after the cheap combined test failed."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _ok(t, dtype, index) -> bool:
    # one short-circuit expression per tensor: ~0.3 us instead of ~0.7 us for the descriptive checks
    return t.dtype is dtype and t.is_cuda and t.get_device() == index and t.is_contiguous()


def _lead(t, name, dtype):
    """the device of the tensor that the other operands of a call have to share it with, after the same two tests"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and _ok(t, dtype, t.get_device())):
        _check_tensor(t, name, dtype)
    return t.device


def _tensor(t, name, dtype, dev, shape=None, style="{0}, got {1}"):
    """t, after the fast test and -- only when that failed -- the slow, precise error; with `shape`, after "<name> must be <style>" too,
    {0} the shape wanted, {1} the shape got and {2} the dtype.  (_ok's expression is repeated here: a call less on every tensor of every
    launch)"""
    if not (t.dtype is dtype and t.is_cuda and t.get_device() == dev.index and t.is_contiguous()):
        _check_tensor(t, name, dtype, dev)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be {style.format(list(shape), list(t.shape), dtype)}")
    return t


def _out(t, name, dtype, dev, shape, style="{0}, got {1}"):
    """this output, checked as _tensor checks it, or a new one of this shape"""
    return torch.empty(shape, dtype=dtype, device=dev) if t is None else _tensor(t, name, dtype, dev, shape, style)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _opt(t):
    return _ptr(t) if t is not None else None


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (saves ~2 us per call)."""
    __slots__ = ("idx", "prev")

    def __init__(self, idx):
        self.idx = idx
        self.prev = -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def _launch(what, dev, entry, *args):
    """the tail of every wrapper: entry(*args) with dev current, a non-zero status raised as `what`'s.  The caller puts
    _stream_ptr(dev) where the entry takes its stream: `args` is then handed on as it is, without a second tuple"""
    with _on_device(dev.index):
        st = entry(*args)
    if st:
        _lib.check(st, what)


def _lib_with(symbol, names, feature):
    """the library, or -- when it was built before `symbol` existed -- what to do about it"""
    lib = _lib.load()
    if not hasattr(lib, symbol):
        raise _lib.MicroMixLibraryError(f"libmicromix_hip.so has no {names}: it was built before {feature}; rebuild it with "
                                        "`python -m micromix_amd.build --force`")
    return lib


def _sf_bytes_w(n, k):   # bindings.cpp:170-172 (rows padded to 128)
    return (n + 127) // 128 * 128 * (k // 32)


def _check_split(KN, KS, KO, K, what):
    """the reference's "Value error in run_<what>" unless (KN, KS, KO) are non-negative multiples of 128 that add up to K (K None: to
    anything but 0)"""
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or (KN + KS + KO != K if K is not None else KN + KS + KO == 0):
        _lib.check(_lib.MM_ERR_BAD_SPLIT, what)


def _round_flags(rounding, integer_round=True):
    if rounding not in ("reference", "fused"):
        raise ValueError("rounding must be 'reference' or 'fused'")
    return (_lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE) | (0 if integer_round else _lib.MM_NORM_NO_INTEGER_ROUND)
