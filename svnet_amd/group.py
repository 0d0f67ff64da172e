"""Ball query and neighbourhood grouping around sampled centres (svnet_amd/csrc/group.hip).

The third point-set helper of the reference's models/utils/pointnet_util.py beside farthest point sampling (svnet_amd/data.py) and
the three-nearest-neighbour interpolation (svnet_amd/propagate.py): `query_ball_point` (lines 87-107) and `sample_and_group` /
`sample_and_group_all` (lines 110-163), the step that turns sampled centres into fixed-size local neighbourhoods - the first level
of a hierarchical encoder, which groups raw coordinates and input attributes.

    new_xyz, new_points = sample_and_group(512, 0.2, 32, xyz, points)           # [B,512,3], [B,512,32,3+D]
    idx, count = query_ball_point(0.2, 32, xyz, new_xyz, return_count=True)     # [B,512,32] int64, [B,512] int32
    grouped = group_points(xyz, new_xyz, idx, points)                           # [B,512,32,3+D]

The contract, for one cloud: points xyz [N,3], centres new_xyz [S,3], optional attributes points [N,D] (channel-last, as the
reference's `sample_and_group` takes them), all fp32.  Every operation is rounded once and never contracted into an fma; fl() is
rounding to fp32.

    distance    d_c = fl(new_xyz[s,c] - xyz[n,c]);   dist[s,n] = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))
                The point-set helpers' one distance, the difference form (svnet_amd/csrc/pointset.h states it and why the reference's
                expanded form is not copied).  On coordinates whose squares and products are exact in fp32 the two forms agree bit
                for bit.
    membership  point n is inside group s when dist[s,n] <= r2 (the reference writes `sqrdists > radius ** 2` -> outside).  r2 is
                an fp32 argument of the C entry point; this layer passes fp32(radius * radius) with the square taken in double, the
                scalar torch's comparison sees.  A NaN distance is never inside.  (Whether torch compares in fp32 or wider does not
                enter any test or recorded case: there r2 is either exact in fp32 - radii 0.125, 0.25, 0.5 - or, for the PointNet++
                radii 0.1, 0.2, 0.4, not a value a distance of lattice coordinates, a multiple of 2^-20, can take, so both
                readings agree.)
    indices     idx [S,nsample] int64: the first nsample inside points in ASCENDING POINT INDEX - what the reference's sort of the
                masked arange(N) yields.  Slots past the number found hold the first inside index (`group_first`).
                count [S] int32 = min(found, nsample); the reference does not return it, a caller that pools over a group wants it.
    empty group no inside point: only when a centre is not one of the points, or a coordinate is not finite.  The reference would
                write index N and fail in `index_points`; HERE count = 0, every slot 0, the rows grouped from point 0 - a stated
                divergence.  Every index written is inside [0, N), always.
    grouping    new_points [S,nsample,3+D]: columns 0..2 = fl(xyz[i,c] - new_xyz[s,c]) (point MINUS centre, line 132), columns 3..
                = points[i,:] copied bit for bit; points=None gives [S,nsample,3].  An index outside [0, N) handed to
                `group_points` is clamped into it, never followed.

On lattice coordinates the whole contract equals the reference's CPU result bit for bit (tests/golden/group.npz; tests/group_ref.py
restates the contract in numpy).

Gradients: `points` may require grad in group_points(), sample_and_group() and sample_and_group_all() - a second set-abstraction
level groups activations.  The grouping then goes through a torch.autograd.Function whose backward is group_points_backward()
(svnet_amd/csrc/pointset_grad.hip):

    backward    with the edges e = s nsample + j that point to n (idx clamped as the forward clamps it) in ascending e,
                e_1 < e_2 < ..., and t_i = dgrouped[s_i,j_i,3+c]:   dpoints[n,c] = fl(fl(fl(t_1 + t_2) + t_3) + ...); one term gives
                t_1, no term +0.  Padded slots and the slots of an empty group are edges like any other.  A fixed order and no
                float atomic: two runs give the same bits (tests/pointset_grad_ref.py restates it).

Coordinates are data: columns 0..2 of the upstream gradient go nowhere, and xyz, new_xyz or idx that require grad are refused, as is
`out=` beside points that require grad.  `Grouper` stays forward only.  There is no CPU fallback: tensors that are not on a HIP
device raise.  Limits: 1 <= nsample <= N <= 32768 (the reference
silently returns N columns when nsample > N; here it is refused), S >= 1, D >= 0, B * ceil(S / 32) <= 2^31 - 1 for the query and
B * S * nsample <= 2^31 - 1 for the grouping; `sample_and_group` also has farthest point sampling's N <= 16384.

Multi-scale grouping (the reference's PointNetSetAbstractionMsg.forward, lines 229-267: the same centres grouped at R radii):

    idx_cat, count = query_ball_point_msg((0.1, 0.2, 0.4), (16, 32, 128), xyz, new_xyz, return_count=True)   # [B,S,176], [B,S,3]
    grouped = group_points_msg(xyz, new_xyz, idx_cat, (16, 32, 128), points)        # R tensors [B,S,nsample_i,D+3]
    new_xyz, grouped = sample_and_group_msg(512, (0.1, 0.2, 0.4), (16, 32, 128), xyz, points)

    query       ONE pass over the cloud for all R radii: a candidate's distance is computed once, every scale that is not yet full
                tests it against its own r2_i = fp32(radius_i * radius_i) and keeps its own list.  idx_cat [S,Ktot] int64 with
                Ktot = sum nsample_i: a centre's row is its R lists end to end, list i at columns off_i .. off_i + nsample_i - 1,
                off_i = nsample_0 + .. + nsample_(i-1) (`split_scales` gives the views); count [S,R] int32.  List i and
                count[:,i] are EXACTLY what query_ball_point(radius_i, nsample_i, ...) returns: the same distance, `<=`, order,
                padding and empty-group rule.  Radii need not be ascending and may repeat (the shorter list of two equal radii is
                then a prefix of the longer).
    grouping    one launch over idx_cat, R separate contiguous tensors [S,nsample_i,D+3] in the reference's Msg order - ATTRIBUTES
                FIRST: columns 0..D-1 = points[i,:] copied bit for bit, columns D..D+2 = fl(xyz[i,c] - new_xyz[s,c]); points=None
                gives [S,nsample_i,3].  (`sample_and_group` writes [xyz | attributes]; the Msg module of the reference does not.)
    backward    group_points_msg_backward: the reverse lists of idx_cat, edges e = s Ktot + j in ascending e - per centre, scale
                0's slots, then scale 1's, ... - and t_i = column c of the upstream gradient of the scale that slot j falls in;
                dpoints[n,c] by the ordered sum above.  No float atomic: two runs give the same bits.
    limits      1 <= R <= 4 (SVNET_MSG_MAX_SCALES), every 1 <= nsample_i <= N <= 32768, S >= 1, D >= 0, B * ceil(S / 32) <= 2^31 - 1
                and B * S * Ktot <= 2^31 - 1; `sample_and_group_msg` also has farthest point sampling's N <= 16384.  The radii and
                nsample travel to the kernels by value: no device copy, no host read, so the calls can be captured.
"""
import numpy as np
import torch

from . import _call, _lib, _pointset
from .data import fps_start

_WHAT = "the grouping"          # in the messages of _pointset.check_tensors


def tile():
    """Points per LDS tile of the ball-query kernel: the N past which its candidate loop takes another tile."""
    return int(_lib.lib().svnet_ball_query_tile())


def _r2(radius):
    """fp32(radius * radius), the square taken in double."""
    radius = float(radius)
    with np.errstate(over="ignore"):          # a square past fp32's range is +inf: every finite distance is inside
        return float(np.float32(radius * radius))


def _with_points(tensors, dtypes, points):
    """(tensors, dtypes) for _pointset.check_tensors, with the optional float32 attributes `points` after them when given."""
    return (tensors, dtypes) if points is None else (dict(tensors, points=points), dtypes + [torch.float32])


def _supported(name, N, S, nsample, D):
    if not _lib.lib().svnet_group_supported(N, S, nsample, D):
        raise _lib.SvnetHipError("%s: N = %d, S = %d, nsample = %d, D = %d is not supported (1 <= nsample <= N <= %d, S >= 1, D >= 0)"
                                 % (name, N, S, nsample, D, _pointset.MAX_N))


def _cloud_shapes(name, xyz, new_xyz):
    return _pointset.check_cloud_pair(name, ("xyz", "new_xyz"), xyz, new_xyz, "NS")


def _points_shape(name, points, B, N):
    if points.dim() != 3 or points.shape[0] != B or points.shape[1] != N:
        raise ValueError("%s: points must be [B,N,D] with B = %d, N = %d, got %s" % (name, B, N, tuple(points.shape)))
    return int(points.shape[2])


def _query_launch(xyz, new_xyz, B, N, S, r2, nsample, idx, count):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_ball_query_f32", _call.p(xyz), _call.p(new_xyz), B, N, S, r2, nsample, _call.p(idx), _call.p(count), _call.stream())


def _group_launch(xyz, new_xyz, points, idx, B, N, S, nsample, D, out):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_group_points_f32", _call.p(xyz), _call.p(new_xyz), _call.p(points if D else None), _call.p(idx), B, N, S, nsample, D,
                  _call.p(out), _call.stream())


def _sample_centres(name, xyz, B, N, S, start, seed=0):
    """What every sampling front end does between its argument checks and its query: resolve `start` (None: data.fps_start(seed, B, N),
    copied from the host; a host array: copied; a device tensor: taken) and check it is [B], farthest point sampling, the gather of
    the centres.  xyz [B,N,3] -> (new_xyz [B,S,3] contiguous, fps_idx [B,S] int64); two launches on the current stream, no host read
    when start is a device tensor.  Errors are raised under the caller's `name`."""
    if start is None:
        start = torch.from_numpy(fps_start(seed, B, N)).to(xyz.device)
    elif not isinstance(start, torch.Tensor):
        start = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int64)).to(xyz.device)
    if tuple(start.shape) != (B,):
        raise ValueError("%s: start must be [B] = [%d], got %s" % (name, B, tuple(start.shape)))
    fps_idx = torch.empty(B, S, dtype=torch.int64, device=xyz.device)
    _pointset.fps_launch(xyz, B, N, S, start, fps_idx)
    return _pointset.gather_rows(xyz, fps_idx).contiguous(), fps_idx


def _cached_start(cache, seed, B, N, device):
    """The default sampling start of a set-abstraction module, data.fps_start(seed, B, N), uploaded once per (seed, B, N, device) and
    kept in the module's `cache` dict."""
    key = (int(seed), B, N, device)
    if key not in cache:
        cache[key] = torch.from_numpy(fps_start(seed, B, N)).to(device)
    return cache[key]


def query_ball_point(radius, nsample, xyz, new_xyz, return_count=False):
    """The reference's name and argument order: xyz [B,N,3], new_xyz [B,S,3] float32 on a HIP device -> idx [B,S,nsample] int64, the
    first nsample points within `radius` of every centre in ascending index, padded with the first (module docstring); with
    return_count also count [B,S] int32.  One launch, no host read; no gradient."""
    _pointset.check_tensors("query_ball_point", {"xyz": xyz, "new_xyz": new_xyz}, (torch.float32, torch.float32), _WHAT)
    B, N, S = _cloud_shapes("query_ball_point", xyz, new_xyz)
    nsample = int(nsample)
    _call.hip(xyz, new_xyz)
    _supported("query_ball_point", N, S, nsample, 0)
    idx = torch.empty(B, S, nsample, dtype=torch.int64, device=xyz.device)
    count = torch.empty(B, S, dtype=torch.int32, device=xyz.device)
    _query_launch(xyz, new_xyz, B, N, S, _r2(radius), nsample, idx, count)
    return (idx, count) if return_count else idx


class _Group(torch.autograd.Function):
    """The grouping launch for points that require grad, and group_points_backward as its backward (current stream, no host read:
    capturable).  xyz, new_xyz and idx get no gradient."""

    @staticmethod
    def forward(ctx, points, xyz, new_xyz, idx):
        (B, N, D), S, nsample = points.shape, idx.shape[1], idx.shape[2]
        out = torch.empty(B, S, nsample, 3 + D, dtype=torch.float32, device=xyz.device)
        _group_launch(xyz, new_xyz, points, idx, B, N, S, nsample, D, out)
        ctx.save_for_backward(idx)
        ctx.N = N
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dgrouped):
        idx, = ctx.saved_tensors
        return group_points_backward(dgrouped.contiguous(), idx, ctx.N), None, None, None


def _group_args(name, xyz, new_xyz, idx, points):
    tensors, dtypes = _with_points({"xyz": xyz, "new_xyz": new_xyz, "idx": idx}, [torch.float32, torch.float32, torch.int64], points)
    _pointset.check_tensors(name, tensors, dtypes, _WHAT, grad=("points",))
    B, N, S = _cloud_shapes(name, xyz, new_xyz)
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != S:
        raise ValueError("%s: idx must be [B,S,nsample] with B = %d, S = %d, got %s" % (name, B, S, tuple(idx.shape)))
    D = 0 if points is None else _points_shape(name, points, B, N)
    return B, N, S, int(idx.shape[2]), D


def group_points(xyz, new_xyz, idx, points=None, out=None):
    """xyz [B,N,3], new_xyz [B,S,3], idx [B,S,nsample] int64, points [B,N,D] or None -> [B,S,nsample,3+D]: the centred coordinates
    of every group's points followed by their attributes (module docstring).  An index outside [0, N) is clamped into it.  One
    launch, no host read; `out` lets a caller keep a fixed buffer.  points may require grad (module docstring); the rest may not."""
    B, N, S, nsample, D = _group_args("group_points", xyz, new_xyz, idx, points)
    _call.hip(xyz, new_xyz, idx, points)
    _supported("group_points", N, S, nsample, D)
    if D and points.requires_grad:
        if out is not None:
            raise ValueError("group_points: out= beside points that require grad - autograd owns the result of a differentiable call")
        return _Group.apply(points, xyz, new_xyz, idx)
    if out is None:
        out = torch.empty(B, S, nsample, 3 + D, dtype=torch.float32, device=xyz.device)
    else:
        _pointset.check_out("group_points", {"xyz": xyz}, out, "[B,S,nsample,3+D]", (B, S, nsample, 3 + D), _WHAT)
    _group_launch(xyz, new_xyz, points, idx, B, N, S, nsample, D, out)
    return out


def group_points_backward(dgrouped, idx, N, out=None):
    """The gradient of group_points with respect to points: dgrouped [B,S,nsample,3+D] float32 (D >= 1), idx [B,S,nsample] int64 ->
    dpoints [B,N,D], the ordered sums of the module docstring.  Two launches on the current stream (the reverse lists of idx, the
    sums), no host read; `out` lets a caller keep a fixed buffer.  Every element of dpoints is written, an empty list as +0."""
    _pointset.check_tensors("group_points_backward", {"dgrouped": dgrouped, "idx": idx}, (torch.float32, torch.int64), _WHAT)
    if idx.dim() != 3 or idx.shape[0] < 1 or dgrouped.dim() != 4 or tuple(dgrouped.shape[:3]) != tuple(idx.shape) or dgrouped.shape[3] < 4:
        raise ValueError("group_points_backward: dgrouped must be [B,S,nsample,3+D] with D >= 1 and idx [B,S,nsample], got %s and %s"
                         % (tuple(dgrouped.shape), tuple(idx.shape)))
    B, S, nsample, D, N = int(idx.shape[0]), int(idx.shape[1]), int(idx.shape[2]), int(dgrouped.shape[3]) - 3, int(N)
    _call.hip(dgrouped, idx)
    _pointset.reverse_supported("group_points_backward", S, nsample, N)
    if out is None:
        out = torch.empty(B, N, D, dtype=torch.float32, device=dgrouped.device)
    else:
        _pointset.check_out("group_points_backward", {"dgrouped": dgrouped}, out, "[B,N,D]", (B, N, D), _WHAT)
    rev_start, rev_edge = _pointset.reverse_lists(idx, N)
    with torch.cuda.device(dgrouped.device):
        _lib.call("svnet_group_points_bwd_f32", _call.p(dgrouped), _call.p(rev_start), _call.p(rev_edge), B, N, S, nsample, D, _call.p(out),
                  _call.stream())
    return out


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, start=None, seed=0):
    """The reference's name and return convention: xyz [B,N,3], points [B,N,D] or None -> (new_xyz [B,npoint,3], new_points
    [B,npoint,nsample,3+D]), with returnfps also (grouped_xyz [B,npoint,nsample,3], the un-centred gather, and fps_idx [B,npoint]).
    Farthest point sampling -> gather of the centres -> ball query -> grouping, on the current stream with no host read between them.
    The reference's torch.randint start is an input, as in data.farthest_point_sample: `start` [B] int64 (a start outside 0 .. N-1 is
    clamped into the cloud by the sampling kernel), or None for data.fps_start(seed, B, N), which is copied from the host: a caller
    that captures the call into a HIP graph passes a device tensor.  points may require grad (module docstring); xyz may not."""
    tensors, dtypes = _with_points({"xyz": xyz}, [torch.float32], points)
    if start is not None and isinstance(start, torch.Tensor):
        tensors["start"] = start
        dtypes.append(torch.int64)
    _pointset.check_tensors("sample_and_group", tensors, dtypes, _WHAT, grad=("points",))
    B, N = _pointset.check_cloud("sample_and_group", "xyz", xyz, "N")
    S, nsample = int(npoint), int(nsample)
    D = 0 if points is None else _points_shape("sample_and_group", points, B, N)
    _call.hip(xyz, points)
    _pointset.fps_supported("sample_and_group", "N", N, S)
    _supported("sample_and_group", N, S, nsample, D)
    new_xyz, fps_idx = _sample_centres("sample_and_group", xyz, B, N, S, start, seed)
    dev = xyz.device
    idx = torch.empty(B, S, nsample, dtype=torch.int64, device=dev)
    count = torch.empty(B, S, dtype=torch.int32, device=dev)
    _query_launch(xyz, new_xyz, B, N, S, _r2(radius), nsample, idx, count)
    if D and points.requires_grad:
        new_points = _Group.apply(points, xyz, new_xyz, idx)
    else:
        new_points = torch.empty(B, S, nsample, 3 + D, dtype=torch.float32, device=dev)
        _group_launch(xyz, new_xyz, points, idx, B, N, S, nsample, D, new_points)
    if not returnfps:
        return new_xyz, new_points
    grouped_xyz = _pointset.gather_rows(xyz, idx.view(B, S * nsample)).view(B, S, nsample, 3)
    return new_xyz, new_points, grouped_xyz, fps_idx


# ---- multi-scale grouping (module docstring: "Multi-scale grouping")
MAX_SCALES = _lib.DEFINES["SVNET_MSG_MAX_SCALES"]


def _scales(name, radius_list, nsample_list):
    """(R, r2 as a C float array or None, nsample as a C int64 array, the nsample tuple) of a call's scales; radius_list=None where
    no radius enters.  The C arrays are host memory the entry points read during the call."""
    nsamples = tuple(int(k) for k in nsample_list)
    R = len(nsamples)
    if radius_list is not None and len(radius_list) != R:
        raise ValueError("%s: %d radii for %d nsample" % (name, len(radius_list), R))
    if not 1 <= R <= MAX_SCALES:
        raise ValueError("%s: %d scales, needs 1 .. %d" % (name, R, MAX_SCALES))
    r2 = None if radius_list is None else (_lib.c_f * R)(*(_r2(r) for r in radius_list))
    return R, r2, (_lib.c_i64 * R)(*nsamples), nsamples


def _supported_msg(name, N, S, R, c_nsample, nsamples, D):
    if not _lib.lib().svnet_group_msg_supported(N, S, R, c_nsample, D):
        raise _lib.SvnetHipError("%s: N = %d, S = %d, nsample = %s, D = %d is not supported (1 .. %d scales, every 1 <= nsample <= N <= %d, "
                                 "S >= 1, D >= 0)" % (name, N, S, list(nsamples), D, MAX_SCALES, _pointset.MAX_N))


def _four(tensors):
    """The pointers of up to four tensors, None past them: the out0 .. out3 / dg0 .. dg3 arguments of the C entry points."""
    return [_call.p(t) for t in tensors] + [None] * (MAX_SCALES - len(tensors))


def _query_msg_launch(xyz, new_xyz, B, N, S, R, c_r2, c_nsample, idx, count):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_ball_query_msg_f32", _call.p(xyz), _call.p(new_xyz), B, N, S, R, c_r2, c_nsample, _call.p(idx), _call.p(count),
                  _call.stream())


def _group_msg_launch(xyz, new_xyz, points, idx_cat, B, N, S, R, c_nsample, nsamples, D, outs=None):
    """-> the R outputs, allocated here unless `outs` (contiguous [B,S,nsample_i,D+3] float32, unchecked: tools/ only) is given."""
    if outs is None:
        outs = [torch.empty(B, S, k, D + 3, dtype=torch.float32, device=xyz.device) for k in nsamples]
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_group_points_msg_f32", _call.p(xyz), _call.p(new_xyz), _call.p(points if D else None), _call.p(idx_cat), B, N, S, R,
                  c_nsample, D, *_four(outs), _call.stream())
    return tuple(outs)


def query_ball_point_msg(radius_list, nsample_list, xyz, new_xyz, return_count=False):
    """query_ball_point for R radii in one pass over the cloud: xyz [B,N,3], new_xyz [B,S,3] -> idx_cat [B,S,Ktot] int64, the R lists
    of a centre end to end (split_scales gives the views), list i exactly query_ball_point(radius_list[i], nsample_list[i], ...);
    with return_count also count [B,S,R] int32.  One launch, no host read; no gradient."""
    _pointset.check_tensors("query_ball_point_msg", {"xyz": xyz, "new_xyz": new_xyz}, (torch.float32, torch.float32), _WHAT)
    B, N, S = _cloud_shapes("query_ball_point_msg", xyz, new_xyz)
    R, c_r2, c_nsample, nsamples = _scales("query_ball_point_msg", radius_list, nsample_list)
    _call.hip(xyz, new_xyz)
    _supported_msg("query_ball_point_msg", N, S, R, c_nsample, nsamples, 0)
    idx = torch.empty(B, S, sum(nsamples), dtype=torch.int64, device=xyz.device)
    count = torch.empty(B, S, R, dtype=torch.int32, device=xyz.device)
    _query_msg_launch(xyz, new_xyz, B, N, S, R, c_r2, c_nsample, idx, count)
    return (idx, count) if return_count else idx


def split_scales(idx_cat, nsample_list):
    """idx_cat [B,S,Ktot] -> the R views [B,S,nsample_i] of its scales (not contiguous: .contiguous() for the single-scale calls)."""
    nsamples = [int(k) for k in nsample_list]
    if idx_cat.dim() != 3 or idx_cat.shape[2] != sum(nsamples):
        raise ValueError("split_scales: idx_cat must be [B,S,%d] for nsample %s, got %s" % (sum(nsamples), nsamples, tuple(idx_cat.shape)))
    return torch.split(idx_cat, nsamples, dim=2)


class _GroupMsg(torch.autograd.Function):
    """The one-launch multi-scale grouping for points that require grad: R outputs, group_points_msg_backward as the backward
    (current stream, no host read: capturable).  xyz, new_xyz and idx_cat get no gradient."""

    @staticmethod
    def forward(ctx, points, xyz, new_xyz, idx_cat, nsamples):
        (B, N, D), S = points.shape, idx_cat.shape[1]
        R, _, c_nsample, _ = _scales("group_points_msg", None, nsamples)
        ctx.save_for_backward(idx_cat)
        ctx.N, ctx.nsamples = N, nsamples
        return _group_msg_launch(xyz, new_xyz, points, idx_cat, B, N, S, R, c_nsample, nsamples, D)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dgrouped):
        idx_cat, = ctx.saved_tensors
        return group_points_msg_backward([g.contiguous() for g in dgrouped], idx_cat, ctx.nsamples, ctx.N), None, None, None, None


def _group_msg_args(name, xyz, new_xyz, idx_cat, nsample_list, points):
    tensors, dtypes = _with_points({"xyz": xyz, "new_xyz": new_xyz, "idx_cat": idx_cat}, [torch.float32, torch.float32, torch.int64], points)
    _pointset.check_tensors(name, tensors, dtypes, _WHAT, grad=("points",))
    B, N, S = _cloud_shapes(name, xyz, new_xyz)
    R, _, c_nsample, nsamples = _scales(name, None, nsample_list)
    if idx_cat.dim() != 3 or idx_cat.shape[0] != B or idx_cat.shape[1] != S or idx_cat.shape[2] != sum(nsamples):
        raise ValueError("%s: idx_cat must be [B,S,Ktot] with B = %d, S = %d, Ktot = %d, got %s" % (name, B, S, sum(nsamples), tuple(idx_cat.shape)))
    D = 0 if points is None else _points_shape(name, points, B, N)
    return B, N, S, R, c_nsample, nsamples, D


def group_points_msg(xyz, new_xyz, idx_cat, nsample_list, points=None):
    """xyz [B,N,3], new_xyz [B,S,3], idx_cat [B,S,Ktot] int64, points [B,N,D] or None -> a tuple of R tensors [B,S,nsample_i,D+3]:
    per scale the attributes of every group's points FOLLOWED BY their centred coordinates (module docstring).  An index outside
    [0, N) is clamped into it.  One launch for all scales, no host read.  points may require grad; the rest may not."""
    B, N, S, R, c_nsample, nsamples, D = _group_msg_args("group_points_msg", xyz, new_xyz, idx_cat, nsample_list, points)
    _call.hip(xyz, new_xyz, idx_cat, points)
    _supported_msg("group_points_msg", N, S, R, c_nsample, nsamples, D)
    if D and points.requires_grad:
        return _GroupMsg.apply(points, xyz, new_xyz, idx_cat, nsamples)
    return _group_msg_launch(xyz, new_xyz, points, idx_cat, B, N, S, R, c_nsample, nsamples, D)


def group_points_msg_backward(dgrouped_list, idx_cat, nsample_list, N, out=None):
    """The gradient of group_points_msg with respect to points: dgrouped_list, R tensors [B,S,nsample_i,D+3] float32 (D >= 1), and
    idx_cat [B,S,Ktot] int64 -> dpoints [B,N,D], the ordered sums of the module docstring.  Two launches on the current stream (the
    reverse lists of idx_cat, the sums), no host read; `out` lets a caller keep a fixed buffer.  Every element is written."""
    dgrouped_list = list(dgrouped_list)
    R, _, c_nsample, nsamples = _scales("group_points_msg_backward", None, nsample_list)
    if len(dgrouped_list) != R:
        raise ValueError("group_points_msg_backward: %d gradients for %d nsample" % (len(dgrouped_list), R))
    tensors = dict({"dgrouped_%d" % i: g for i, g in enumerate(dgrouped_list)}, idx_cat=idx_cat)
    _pointset.check_tensors("group_points_msg_backward", tensors, [torch.float32] * R + [torch.int64], _WHAT)
    W = int(dgrouped_list[0].shape[-1]) if dgrouped_list[0].dim() == 4 else 0
    if idx_cat.dim() != 3 or idx_cat.shape[0] < 1 or idx_cat.shape[2] != sum(nsamples) or W < 4 or any(
            tuple(g.shape) != (idx_cat.shape[0], idx_cat.shape[1], k, W) for g, k in zip(dgrouped_list, nsamples)):
        raise ValueError("group_points_msg_backward: dgrouped_list must be [B,S,nsample_i,D+3] with D >= 1 for nsample %s and idx_cat "
                         "[B,S,%d], got %s and %s" % (list(nsamples), sum(nsamples), [tuple(g.shape) for g in dgrouped_list], tuple(idx_cat.shape)))
    B, S, D, N = int(idx_cat.shape[0]), int(idx_cat.shape[1]), W - 3, int(N)
    _call.hip(idx_cat, *dgrouped_list)
    _supported_msg("group_points_msg_backward", N, S, R, c_nsample, nsamples, D)
    _pointset.reverse_supported("group_points_msg_backward", S, sum(nsamples), N)
    if out is None:
        out = torch.empty(B, N, D, dtype=torch.float32, device=idx_cat.device)
    else:
        _pointset.check_out("group_points_msg_backward", {"dgrouped_0": dgrouped_list[0]}, out, "[B,N,D]", (B, N, D), _WHAT)
    rev_start, rev_edge = _pointset.reverse_lists(idx_cat, N)
    with torch.cuda.device(idx_cat.device):
        _lib.call("svnet_group_points_msg_bwd_f32", *_four(dgrouped_list), _call.p(rev_start), _call.p(rev_edge), B, N, S, R, c_nsample, D,
                  _call.p(out), _call.stream())
    return out


def sample_and_group_msg(npoint, radius_list, nsample_list, xyz, points, start=None, seed=0):
    """The sampling and grouping of the reference's PointNetSetAbstractionMsg.forward: xyz [B,N,3], points [B,N,D] or None ->
    (new_xyz [B,npoint,3], a tuple of R tensors [B,npoint,nsample_i,D+3]).  Farthest point sampling -> gather of the centres -> the
    one-pass query -> the one-launch grouping, on the current stream with no host read between them.  `start` and `seed` as in
    sample_and_group: a caller that captures the call passes a device tensor.  points may require grad; xyz may not."""
    tensors, dtypes = _with_points({"xyz": xyz}, [torch.float32], points)
    if start is not None and isinstance(start, torch.Tensor):
        tensors["start"] = start
        dtypes.append(torch.int64)
    _pointset.check_tensors("sample_and_group_msg", tensors, dtypes, _WHAT, grad=("points",))
    B, N = _pointset.check_cloud("sample_and_group_msg", "xyz", xyz, "N")
    S = int(npoint)
    R, c_r2, c_nsample, nsamples = _scales("sample_and_group_msg", radius_list, nsample_list)
    D = 0 if points is None else _points_shape("sample_and_group_msg", points, B, N)
    _call.hip(xyz, points)
    _pointset.fps_supported("sample_and_group_msg", "N", N, S)
    _supported_msg("sample_and_group_msg", N, S, R, c_nsample, nsamples, D)
    new_xyz, _ = _sample_centres("sample_and_group_msg", xyz, B, N, S, start, seed)
    dev = xyz.device
    idx = torch.empty(B, S, sum(nsamples), dtype=torch.int64, device=dev)
    count = torch.empty(B, S, R, dtype=torch.int32, device=dev)
    _query_msg_launch(xyz, new_xyz, B, N, S, R, c_r2, c_nsample, idx, count)
    if D and points.requires_grad:
        return new_xyz, _GroupMsg.apply(points, xyz, new_xyz, idx, nsamples)
    return new_xyz, _group_msg_launch(xyz, new_xyz, points, idx, B, N, S, R, c_nsample, nsamples, D)


def sample_and_group_all(xyz, points):
    """The reference's trivial form: one group of all N points around centre 0, in order.  xyz [B,N,3], points [B,N,D] or None ->
    (new_xyz [B,1,3] of zeros, new_points [B,1,N,3+D]).  torch views and one cat, so torch's own autograd carries the gradient of
    points, which may require grad; xyz may not."""
    _pointset.check_tensors("sample_and_group_all", *_with_points({"xyz": xyz}, [torch.float32], points), _WHAT, grad=("points",))
    B, N = _pointset.check_cloud("sample_and_group_all", "xyz", xyz, "N")
    if points is not None:
        _points_shape("sample_and_group_all", points, B, N)
    _call.hip(xyz, points)
    new_xyz = torch.zeros(B, 1, 3, dtype=torch.float32, device=xyz.device)
    grouped = xyz.view(B, 1, N, 3)
    return new_xyz, (grouped if points is None else torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1))


class Grouper:
    """query_ball_point() + group_points() on buffers allocated once: idx [B,S,nsample], count [B,S] and out [B,S,nsample,3+D] for
    up to B clouds.  run(xyz, new_xyz, radius, points) takes the first `count` clouds of each and returns out[:count] (the indices
    and counts of that call are in .idx[:count] / .count[:count]); nothing is allocated per call."""

    def __init__(self, B, N, S, nsample, D, device):
        device = _pointset.hip_device("Grouper", device)
        self.B, self.N, self.S, self.nsample, self.D = int(B), int(N), int(S), int(nsample), int(D)
        if self.B < 1:
            raise ValueError("Grouper: B = %d < 1" % self.B)
        _supported("Grouper", self.N, self.S, self.nsample, self.D)
        self.idx = torch.empty(self.B, self.S, self.nsample, dtype=torch.int64, device=device)
        self.count = torch.empty(self.B, self.S, dtype=torch.int32, device=device)
        self.out = torch.empty(self.B, self.S, self.nsample, 3 + self.D, dtype=torch.float32, device=device)

    def run(self, xyz, new_xyz, radius, points=None):
        _pointset.check_tensors("Grouper.run", *_with_points({"xyz": xyz, "new_xyz": new_xyz}, [torch.float32, torch.float32], points), _WHAT)
        count, N, S = _cloud_shapes("Grouper.run", xyz, new_xyz)
        D = 0 if points is None else _points_shape("Grouper.run", points, count, N)
        _call.hip(xyz, new_xyz, points)
        if count > self.B or (N, S, D) != (self.N, self.S, self.D) or xyz.device != self.out.device:
            raise ValueError("Grouper.run: xyz %s, new_xyz %s, points %s do not fit B <= %d, N %d, S %d, D %d on %s"
                             % (tuple(xyz.shape), tuple(new_xyz.shape), None if points is None else tuple(points.shape), self.B, self.N,
                                self.S, self.D, self.out.device))
        _query_launch(xyz, new_xyz, count, N, S, _r2(radius), self.nsample, self.idx, self.count)
        _group_launch(xyz, new_xyz, points, self.idx, count, N, S, self.nsample, D, self.out)
        return self.out[:count]
