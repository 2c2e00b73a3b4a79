"""A stand-in torch for the tests that drive Hip's Python entry points without a GPU: tensors with host memory behind them (as the stand-in
runtime's hipMalloc, tests/stubs/fakehip.c), one stream and a device context that does nothing. install() puts it into sys.modules["torch"].

Tensor.count counts the float32 torch.empty calls (the films of a sequence; scratch buffers are bytes, outputs come from empty_like).
With Tensor.events set to a list, every allocation (empty, zeros, empty_like, zeros_like: shape and dtype), zero_() and synchronize() is
appended to it, and every tensor is kept alive, so that an address names one tensor: number(ptr) gives the small running number of the tensor
that holds the address, counted from the first time it is asked for. Conversions (from_numpy, to, contiguous, clone, reshape) are no events."""
import sys
import types

import numpy as np


class Tensor:
    count = 0
    events = None
    _alive, _numbers = [], {}

    def __init__(self, a):
        self.a = a; self.shape = a.shape; self.device = "cuda:0"
        if Tensor.events is not None:
            Tensor._alive.append(self)

    def data_ptr(self): return self.a.ctypes.data
    def dim(self): return self.a.ndim
    def to(self, *a): return self
    def contiguous(self): return self
    def clone(self): return Tensor(self.a.copy())
    def reshape(self, *s): return Tensor(self.a.reshape(*s))
    def cpu(self): return self
    def numpy(self): return self.a
    def __add__(self, other): return Tensor(self.a + other.a)

    def zero_(self):
        self.a[...] = 0
        _event("zero_", number(self.data_ptr()))
        return self


def _event(*what):
    if Tensor.events is not None:
        Tensor.events.append(list(what))


def number(ptr):
    """the running number of the tensor at this address, or None where no tensor made since record() lives there"""
    if ptr not in Tensor._numbers:
        if not any(t.data_ptr() == ptr for t in Tensor._alive):
            return None
        Tensor._numbers[ptr] = len(Tensor._numbers)
    return Tensor._numbers[ptr]


def record():
    """start a fresh list of events and a fresh numbering; returns the list"""
    Tensor.events, Tensor._alive, Tensor._numbers = [], [], {}
    return Tensor.events


class Stream:
    cuda_stream = 0x5150

    def synchronize(self): _event("synchronize")


class Ctx:
    def __enter__(self): return self
    def __exit__(self, *a): return False


def _allocate(name, array, dtype):
    t = Tensor(array)
    _event(name, list(t.shape), np.dtype(dtype).name, number(t.data_ptr()))
    return t


def fake_torch():
    torch = types.ModuleType("torch")
    torch.float32, torch.uint8 = np.float32, np.uint8
    torch.from_numpy = lambda a: Tensor(a)

    def empty(shape, dtype=None, device=None):
        Tensor.count += dtype is np.float32
        return _allocate("empty", np.zeros(shape, dtype), dtype)
    torch.empty = empty
    torch.zeros = lambda shape, dtype=None, device=None: _allocate("zeros", np.zeros(shape, dtype), dtype)
    torch.empty_like = lambda t: _allocate("empty_like", np.zeros_like(t.a), t.a.dtype)
    torch.zeros_like = lambda t: _allocate("zeros_like", np.zeros_like(t.a), t.a.dtype)
    torch.device = lambda d: d
    torch.cuda = types.SimpleNamespace(device=lambda d: Ctx(), current_stream=lambda: Stream())
    return torch


def install():
    sys.modules["torch"] = fake_torch()
