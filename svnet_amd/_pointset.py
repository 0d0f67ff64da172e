"""What the front ends of the point-set helpers share: farthest point sampling (svnet_amd/data.py), the three-nearest-neighbour
propagation (svnet_amd/propagate.py), ball query and grouping (svnet_amd/group.py).  Private: the public names live in those modules.
The device side of the same contract - the distance all three use, the LDS tile, the launch geometry - is svnet_amd/csrc/pointset.h.

Here: the argument checks in the order every entry point applies them (tensors, then shapes, then - by _ops._hip - the HIP device,
then the kernels' limits), the device refusal of the classes that allocate, the row gather, and the one launch of the sampler.
"""
import torch

from . import _lib, _ops

MAX_N = 32768       # SVNET_KNN_MAX_N (svnet_amd/csrc/common.h), for the messages: the library's *_supported queries are the check


def check_tensors(name, tensors, dtypes, what):
    """tensors: {argument name: tensor}; the type, dtype, device-match, contiguity and no-gradient checks shared by the entry points
    (the HIP device itself is checked after the shapes, by _ops._hip).  `what` names the operation: "the grouping"."""
    for k, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (name, k, type(t).__name__))
    for (k, t), dt in zip(tensors.items(), dtypes):
        if t.dtype != dt:
            raise TypeError("%s: %s must be %s, got %s" % (name, k, dt, t.dtype))
    first = next(iter(tensors.values()))
    for k, t in tensors.items():
        if t.device != first.device:
            raise ValueError("%s: %s on %s, %s on %s" % (name, next(iter(tensors)), first.device, k, t.device))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (name, k))
        if t.requires_grad:
            raise ValueError("%s: %s requires grad - %s is forward only" % (name, k, what))


def check_cloud(name, arg, t, letter):
    """t must be [B,<letter>,3] with B >= 1 -> (B, points per cloud)."""
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1:
        raise ValueError("%s: %s must be [B,%s,3], got %s" % (name, arg, letter, tuple(t.shape)))
    return int(t.shape[0]), int(t.shape[1])


def check_cloud_pair(name, args, a, b, letters):
    """a [B,<letters[0]>,3] and b [B,<letters[1]>,3] of the same B, named args[0] and args[1] -> (B, points of a, points of b)."""
    B, n = check_cloud(name, args[0], a, letters[0])
    if b.dim() != 3 or b.shape[2] != 3 or b.shape[0] != B:
        raise ValueError("%s: %s must be [B,%s,3] with B = %d, got %s" % (name, args[1], letters[1], B, tuple(b.shape)))
    return B, n, int(b.shape[1])


def check_out(name, beside, out, layout, shape, what):
    """A caller's `out` buffer: float32, contiguous, without gradient, on the device of the input `beside` ({argument name: tensor}),
    and of exactly `shape`, which the message spells as `layout`."""
    check_tensors(name, dict(beside, out=out), (torch.float32, torch.float32), what)
    if tuple(out.shape) != shape:
        raise ValueError("%s: out must be %s = %s, got %s" % (name, layout, shape, tuple(out.shape)))


def hip_device(who, device):
    """torch.device(device), refused unless it is a HIP (cuda) device: for the classes that allocate on it."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("svnet_amd: %s needs a HIP (cuda) device, got %s — the product path has no CPU fallback" % (who, device))
    return device


def gather_rows(x, idx):
    """x [B,N,3], idx [B,S] int64 -> [B,S,3]: x[b, idx[b,s], :]."""
    return torch.gather(x, 1, idx.unsqueeze(2).expand(-1, -1, 3))


def fps_supported(name, letter, P, npoint):
    """The sampler's limits (a lane keeps at most 16 points: svnet_amd/csrc/fps.hip); `letter` is the caller's name for P."""
    if not _lib.lib().svnet_fps_supported(P, npoint):
        raise _lib.SvnetHipError("%s: %s = %d, npoint = %d is not supported (1 <= npoint <= %s <= 16384)" % (name, letter, P, npoint, letter))


def fps_launch(xyz, B, P, npoint, start, idx):
    """The sampler on the current stream: xyz [B,P,3], start [B] int64 -> idx [B,npoint] int64 (given).  No host read: capturable.
    A start outside 0 .. P-1 is clamped into the cloud by the kernel; callers that refuse it check before."""
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_fps_f32", _ops._p(xyz), B, P, npoint, _ops._p(start), _ops._p(idx), _ops._stream())
