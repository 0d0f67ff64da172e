"""What every front end needs to call the C ABI (include/svnet_hip.h) with torch tensors: the data pointer of a tensor, the
current HIP stream, the device and dtype checks, and `call` itself.  A leaf: torch, ctypes and _lib, nothing else of the package.
Use it through the module (`_call.hip(...)`): the names are looked up at call time, so a test can replace one by attribute.
"""
import ctypes

import torch

from ._lib import call          # noqa: F401  (re-exported: _call.call)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("svnet_amd: expected a HIP (cuda) tensor, got %s — the product path has no CPU fallback" % t.device)


def f32c(t):
    if t.dtype != torch.float32:
        raise TypeError("svnet_amd: expected float32, got %s" % t.dtype)
    return t if t.is_contiguous() else t.contiguous()
