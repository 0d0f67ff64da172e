"""What the front ends of the point-set helpers share: farthest point sampling (svnet_amd/data.py), the three-nearest-neighbour
propagation (svnet_amd/propagate.py), ball query and grouping (svnet_amd/group.py).  Private: the public names live in those modules.
The device side of the same contract - the distance all three use, the LDS tile, the launch geometry - is svnet_amd/csrc/pointset.h.

Here: the argument checks in the order every entry point applies them (tensors, then shapes, then - by _call.hip - the HIP device,
then the kernels' limits), the device refusal of the classes that allocate, the row gather, the one launch of the sampler, and the
reverse lists both backwards sum over (svnet_amd/csrc/pointset_grad.hip).
"""
import torch

from . import _call, _lib

MAX_N = 32768       # SVNET_KNN_MAX_N (svnet_amd/csrc/common.h), for the messages: the library's *_supported queries are the check


def check_tensors(name, tensors, dtypes, what, grad=()):
    """tensors: {argument name: tensor}; the type, dtype, device-match, contiguity and gradient checks shared by the entry points
    (the HIP device itself is checked after the shapes, by _call.hip).  `what` names the operation: "the grouping".  `grad` names
    the arguments that may require grad - the data tensors whose backward exists, on a HIP device; coordinates, weights and indices
    never may.  Returns whether one of them does."""
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
        if t.requires_grad and k not in grad:
            raise ValueError("%s: %s requires grad - %s is forward only in %s" % (name, k, what, k))
        if t.requires_grad and t.device.type != "cuda":
            raise ValueError("%s: %s requires grad on %s - off a HIP device %s is forward only" % (name, k, t.device, what))
    return any(tensors[k].requires_grad for k in grad if k in tensors)


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


def rows(t):
    """[B,C,N] channel-first, as the modules take clouds and features -> [B,N,C] contiguous, as the kernels do (autograd follows)."""
    return t.permute(0, 2, 1).contiguous()


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
        _lib.call("svnet_fps_f32", _call.p(xyz), B, P, npoint, _call.p(start), _call.p(idx), _call.stream())


def reverse_supported(name, R, K, N):
    if not _lib.lib().svnet_pointset_reverse_supported(R, K, N):
        raise _lib.SvnetHipError("%s: a [%d,%d] index table into N = %d points is not supported (1 <= N <= %d, 1 <= R * K <= 2^31 - 1)"
                                 % (name, R, K, N, MAX_N))


def reverse_tile():
    """Destinations one workgroup of the reverse-list builder owns (a quarter of them per wave): the N past which a cloud takes a
    second workgroup."""
    return int(_lib.lib().svnet_pointset_reverse_tile())


def reverse_chunk():
    """Edges per LDS chunk of the reverse-list builder: the R * K past which its edge loop takes a second chunk."""
    return int(_lib.lib().svnet_pointset_reverse_chunk())


def reverse_lists(idx, N):
    """idx [B,R,K] int64 on a HIP device with targets in [0, N) (clamped into it, as the forward kernels do) -> (rev_start [B,N+1],
    rev_edge [B,R*K]) int32: per cloud, rev_edge[rev_start[n] : rev_start[n+1]] are the edges e = r K + j that point to n, in
    ascending e; nothing is skipped.  One launch on the current stream, no host read: capturable."""
    B, R, K = (int(v) for v in idx.shape)
    N = int(N)
    reverse_supported("reverse_lists", R, K, N)
    rev_start = torch.empty(B, N + 1, dtype=torch.int32, device=idx.device)
    rev_edge = torch.empty(B, R * K, dtype=torch.int32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.call("svnet_pointset_reverse_i32", _call.p(idx), B, R, K, N, _call.p(rev_start), _call.p(rev_edge), _call.stream())
    return rev_start, rev_edge
