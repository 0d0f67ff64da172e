"""Fused set-abstraction level for inference: grouping, the shared MLP and the max over a group as one launch
(svnet_amd/csrc/sa_fused.hip).

In eval mode everything a set-abstraction level does after the ball query is a pure function of one centre's group: gather `nsample`
rows, run two to four 1x1 convolutions with BatchNorm's running statistics and ReLU, take the maximum.  The modules of
svnet_amd/models/utils (pointnet_util.py, pointnet_msg.py) write the grouped tensor [B,S,nsample,3+D] and every layer's activation to
memory; here nothing leaves the compute unit but C_out floats per centre.  Training is out of scope (batch statistics need a barrier
after every layer, the backward needs the activations): the modules stay as they are, this is an entry beside them.

    level = fold_level(module.mlp_convs, module.mlp_bns)                        # buffers allocated once; level.refresh() re-folds
    out = group_mlp_max(xyz, new_xyz, idx, points, level, count=count)          # [B,C_out,S]
    fused = FusedSetAbstraction(module)                                         # PointNetSetAbstraction or PointNetSetAbstractionMsg
    new_xyz, new_points = fused(xyz, points)                                    # the module's eval-mode forward

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf):

    fold        per layer, from the convolution W [O,C], b [O] and BatchNorm's gamma, beta, running_mean, running_var [O]:
                invstd[o] = fl(1 / fl(sqrt(fl(var[o] + eps))));  s[o] = fl(gamma[o] invstd[o]);  Wf[o,c] = fl(W[o,c] s[o]);
                bf[o] = fl(fl(fl(b[o] - mean[o]) s[o]) + beta[o]).  One launch per layer, no host read.
    rows        row j of centre s: n = idx[s,j] clamped into 0 .. N-1; h0 = [fl(xyz[n,c] - new_xyz[s,c]) | points[n,:]], or
                [points[n,:] | the differences] with xyz_last (the multi-scale order); the attributes bit for bit.
    layers      per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc if acc > 0 else +0.
                The bias is the accumulator's start and K is never split, so no value depends on how the kernel tiles rows, columns
                or centres (the products run on v_mfma_f32_16x16x4_f32, bit for bit this chain).
    output      out[c_off + o, s] = max_j hL_j[o], channel-first into [C_total,S]: the scales of a multi-scale level land in the
                concatenated result, the other channels are left alone.
    count       with count [S] the slots >= max(count[s], 1) are skipped: they repeat slot 0 (the query's padding; an empty group is
                nsample copies of point 0), so the result is that of all slots.
    limits      1 <= K <= N <= 32768, S >= 1, 0 <= D <= 321, 1 .. 4 layers of width 1 .. 256 (`supported`).  Inputs are assumed finite.

tests/sa_fused_ref.py restates the contract in numpy; the results are compared as bit patterns (a -0 counted as +0).  No argument may
require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _level, _lib, _pointset
from ._level import MAX_LAYERS, FoldedLevel, fold_level
from .group import _query_msg_launch, _sample_centres, _scales

__all__ = ["FoldedLevel", "fold_level", "group_mlp_max", "supported", "rows_tile", "FusedSetAbstraction"]

_WHAT = "the fused set-abstraction level"          # in the messages of _pointset.check_tensors
_F32 = torch.float32


def rows_tile():
    """Grouped rows one workgroup multiplies at a time: a group of more slots takes further tiles, smaller groups share one."""
    return int(_lib.lib().svnet_sa_fused_rows_tile())


def supported(N, S, K, D, widths):
    """Whether the fused kernel takes this level (module docstring, limits)."""
    return bool(_lib.lib().svnet_sa_fused_supported(int(N), int(S), int(K), int(D), *_level.c_widths(widths)))


def _launch(xyz, new_xyz, idx, idx_ld, points, level, count, count_ld, xyz_last, out, c_off, B, N, S, K, D):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_sa_fused_f32", _call.p(xyz), _call.p(new_xyz), _call.p(points if D else None), _call.p(idx), idx_ld, _call.p(count),
                  count_ld, B, N, S, K, D, len(level.widths), level._c_widths, level._c_wf, level._c_bf, int(bool(xyz_last)), _call.p(out),
                  int(out.shape[1]), c_off, _call.stream())


def _row_stride(name, arg, t, inner):
    """t [B,S,inner] (idx) or [B,S] with inner = 1 (count): unit stride along the last axis of idx, rows `ld` >= inner elements apart
    and clouds S * ld apart - a contiguous tensor, or a slice of the last axis of one (a scale's columns of a concatenated table) -> ld."""
    B, S, st = int(t.shape[0]), int(t.shape[1]), t.stride()
    ld = int(st[1]) if S > 1 else int(st[0]) if B > 1 else inner
    if not ((t.dim() == 2 or inner == 1 or st[2] == 1) and ld >= inner and (B == 1 or st[0] == S * ld)):
        raise ValueError("%s: %s must be contiguous, or a slice of the last axis of a contiguous tensor; its strides are %s" % (name, arg, tuple(st)))
    return ld


def group_mlp_max(xyz, new_xyz, idx, points, level, count=None, xyz_last=False, out=None, c_off=0):
    """xyz [B,N,3], new_xyz [B,S,3], idx [B,S,K] int64, points [B,N,D] or None, level a FoldedLevel for 3 + D input columns ->
    out [B,C_total,S] with channels c_off .. c_off + C_out - 1 written (module docstring); out=None allocates [B,C_out,S].  idx and
    count [B,S] int32 may be slices of the last axis of a contiguous tensor - a scale's columns of query_ball_point_msg's table and
    counts.  One launch on the current stream, no host read, no workspace.  No argument may require grad."""
    name = "group_mlp_max"
    _level.check_is_level(name, level, "fold_level")
    _level.check_args(name, _WHAT, {"xyz": (xyz, _F32), "new_xyz": (new_xyz, _F32)}, {"points": (points, _F32), "out": (out, _F32)})
    strided = {"idx": (idx, torch.int64)}
    if count is not None:
        strided["count"] = (count, torch.int32)
    for k, (t, dt) in strided.items():                     # check_tensors' checks but the contiguity: _row_stride below
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (name, k, type(t).__name__))
        if t.dtype != dt:
            raise TypeError("%s: %s must be %s, got %s" % (name, k, dt, t.dtype))
        if t.device != xyz.device:
            raise ValueError("%s: xyz on %s, %s on %s" % (name, xyz.device, k, t.device))
    B, N, S = _pointset.check_cloud_pair(name, ("xyz", "new_xyz"), xyz, new_xyz, "NS")
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != S or idx.shape[2] < 1:
        raise ValueError("%s: idx must be [B,S,K] with B = %d, S = %d, got %s" % (name, B, S, tuple(idx.shape)))
    K = int(idx.shape[2])
    idx_ld = _row_stride(name, "idx", idx, K)
    if count is not None and tuple(count.shape) != (B, S):
        raise ValueError("%s: count must be [B,S] = %s, got %s" % (name, (B, S), tuple(count.shape)))
    count_ld = 0 if count is None else _row_stride(name, "count", count, 1)
    D = 0
    if points is not None:
        if points.dim() != 3 or points.shape[0] != B or points.shape[1] != N:
            raise ValueError("%s: points must be [B,N,D] with B = %d, N = %d, got %s" % (name, B, N, tuple(points.shape)))
        D = int(points.shape[2])
    _level.check_c_in(name, level, 3 + D, "xyz and points give 3 + %d" % D)
    c_off = _level.check_window(name, out, c_off, level, B, S, "S")
    _call.hip(xyz, new_xyz, idx, points, count, out)
    _level.check_device(name, level, "xyz", xyz)
    if not supported(N, S, K, D, level.widths):
        raise _lib.SvnetHipError("%s: N = %d, S = %d, K = %d, D = %d, widths %s is not supported (1 <= K <= N <= %d, S >= 1, D <= 321, 1 .. %d "
                                 "layers of width 1 .. 256)" % (name, N, S, K, D, list(level.widths), _pointset.MAX_N, MAX_LAYERS))
    out = _level.result(out, level, B, S, xyz.device)
    _launch(xyz, new_xyz, idx, idx_ld, points, level, count, count_ld, xyz_last, out, c_off, B, N, S, K, D)
    return out


class FusedSetAbstraction(_level.FusedWrapper):
    """The eval-mode forward of a PointNetSetAbstraction (group_all=False) or a PointNetSetAbstractionMsg on a HIP device, with the
    module's signature, default start and results:

        fused(xyz [B,3,N], points [B,D,N] or None, start=None) -> (new_xyz [B,3,S], new_points [B,C,S])

    Farthest point sampling -> gather of the centres -> ONE query pass for all scales -> ONE fused launch per scale, which writes its
    channels of the concatenated result: on the current stream, no host read (a caller that captures the call passes a device
    `start`), under no_grad.  The layers are folded at construction; refresh() folds them again after the module's parameters or
    running statistics changed.  A module in train mode is refused: batch statistics are not what this computes.  A level outside
    the kernel's limits (`supported`) goes through the module's own forward."""

    def __init__(self, module):
        from .models.utils.pointnet_msg import PointNetSetAbstractionMsg
        from .models.utils.pointnet_util import PointNetSetAbstraction
        if isinstance(module, PointNetSetAbstraction):
            if module.group_all:
                raise ValueError("FusedSetAbstraction: a group_all level has no query to fuse behind - that level is sa_global.FusedGlobalAbstraction's")
            self.radii, self.nsamples, self.xyz_last = (module.radius,), (int(module.nsample),), False
            self.levels = [fold_level(module.mlp_convs, module.mlp_bns)]
        elif isinstance(module, PointNetSetAbstractionMsg):
            self.radii, self.nsamples, self.xyz_last = tuple(module.radius_list), tuple(int(k) for k in module.nsample_list), True
            self.levels = [fold_level(convs, bns) for convs, bns in zip(module.conv_blocks, module.bn_blocks)]
        else:
            raise TypeError("FusedSetAbstraction: needs a PointNetSetAbstraction or a PointNetSetAbstractionMsg, got %s" % type(module).__name__)
        self.module, self.npoint = module, int(module.npoint)
        self.channels = sum(level.widths[-1] for level in self.levels)

    def supported(self, N, D):
        """Whether clouds of N points with D attributes take the fused path here; else __call__ runs the module."""
        R, _, c_nsample, _ = _scales("FusedSetAbstraction", self.radii, self.nsamples)
        lib = _lib.lib()
        return bool(lib.svnet_fps_supported(N, self.npoint) and lib.svnet_group_msg_supported(N, self.npoint, R, c_nsample, D)
                    and all(level.c_in == 3 + D and supported(N, self.npoint, k, D, level.widths)
                            for level, k in zip(self.levels, self.nsamples)))

    @torch.no_grad()
    def __call__(self, xyz, points, start=None):
        name = self._begin(_WHAT, {"xyz": (xyz, _F32)}, {"points": (points, _F32), "start": (start, torch.int64)})
        B, N, D = _level.cloud_shapes(name, xyz, points)
        _call.hip(xyz, points, start)
        if not self.supported(N, D):
            return self.module(xyz, points, start=start)
        if start is None:
            start = self.module._start(B, N, xyz.device)
        dev, S = xyz.device, self.npoint
        rows, attrs = _pointset.rows(xyz), None if points is None else _pointset.rows(points)
        R, c_r2, c_nsample, nsamples = _scales(name, self.radii, self.nsamples)
        new_xyz, _ = _sample_centres(name, rows, B, N, S, start)
        Ktot = sum(nsamples)
        idx = torch.empty(B, S, Ktot, dtype=torch.int64, device=dev)
        count = torch.empty(B, S, R, dtype=torch.int32, device=dev)
        _query_msg_launch(rows, new_xyz, B, N, S, R, c_r2, c_nsample, idx, count)
        out = torch.empty(B, self.channels, S, dtype=torch.float32, device=dev)
        off = c_off = 0
        for i, (level, k) in enumerate(zip(self.levels, nsamples)):
            _launch(rows, new_xyz, idx[:, :, off:], Ktot, attrs, level, count[:, :, i:], R, self.xyz_last, out, c_off, B, N, S, k, D)
            off += k
            c_off += level.widths[-1]
        return new_xyz.permute(0, 2, 1), out
