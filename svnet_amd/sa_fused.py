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

from . import _lib, _ops, _pointset
from .group import _query_msg_launch, _sample_centres, _scales

__all__ = ["FoldedLevel", "fold_level", "group_mlp_max", "supported", "rows_tile", "FusedSetAbstraction"]

_WHAT = "the fused set-abstraction level"          # in the messages of _pointset.check_tensors
MAX_LAYERS = _lib.DEFINES["SVNET_SA_MAX_LAYERS"]


def rows_tile():
    """Grouped rows one workgroup multiplies at a time: a group of more slots takes further tiles, smaller groups share one."""
    return int(_lib.lib().svnet_sa_fused_rows_tile())


def supported(N, S, K, D, widths):
    """Whether the fused kernel takes this level (module docstring, limits)."""
    widths = [int(w) for w in widths]
    return bool(_lib.lib().svnet_sa_fused_supported(int(N), int(S), int(K), int(D), len(widths), (_lib.c_i64 * max(len(widths), 1))(*widths)))


class FoldedLevel:
    """The folded layers of one level: Wf_l [C_l, C_(l-1)] and bf_l [C_l] on the layers' device, allocated once.  refresh() runs the
    folds again - after the parameters or the running statistics changed - on the current stream, one launch per layer."""

    def __init__(self, convs, bns):
        convs, bns = list(convs), list(bns)
        if len(convs) != len(bns) or not 1 <= len(convs) <= MAX_LAYERS:
            raise ValueError("fold_level: %d convolutions and %d BatchNorms, needs 1 .. %d pairs" % (len(convs), len(bns), MAX_LAYERS))
        last = None
        for i, (conv, bn) in enumerate(zip(convs, bns)):
            w = conv.weight
            if w.dim() < 2 or any(int(v) != 1 for v in w.shape[2:]) or conv.bias is None:
                raise ValueError("fold_level: layer %d must be a 1x1 convolution with a bias, got a weight of %s" % (i, tuple(w.shape)))
            if bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
                raise ValueError("fold_level: BatchNorm %d must be affine and track running statistics" % i)
            if int(bn.num_features) != int(w.shape[0]) or (last is not None and int(w.shape[1]) != last):
                raise ValueError("fold_level: layer %d is %s, BatchNorm over %d, behind a layer of width %s"
                                 % (i, tuple(w.shape), bn.num_features, last))
            tensors = {"weight": w, "bias": conv.bias, "bn.weight": bn.weight, "bn.bias": bn.bias, "running_mean": bn.running_mean,
                       "running_var": bn.running_var}
            for k, t in tensors.items():
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != w.device:
                    raise ValueError("fold_level: layer %d %s must be contiguous float32 on %s" % (i, k, w.device))
            last = int(w.shape[0])
        self.device = _pointset.hip_device("fold_level", convs[0].weight.device)
        self.convs, self.bns = convs, bns
        self.c_in = int(convs[0].weight.shape[1])
        self.widths = tuple(int(c.weight.shape[0]) for c in convs)
        self.wf = [torch.empty(int(c.weight.shape[0]), int(c.weight.shape[1]), dtype=torch.float32, device=self.device) for c in convs]
        self.bf = [torch.empty(w, dtype=torch.float32, device=self.device) for w in self.widths]
        L = len(convs)
        self._c_widths = (_lib.c_i64 * L)(*self.widths)
        self._c_wf = (_lib.c_p * L)(*(t.data_ptr() for t in self.wf))
        self._c_bf = (_lib.c_p * L)(*(t.data_ptr() for t in self.bf))
        self.refresh()

    def refresh(self):
        with torch.cuda.device(self.device):
            for conv, bn, wf, bf in zip(self.convs, self.bns, self.wf, self.bf):
                if conv.weight.device != self.device:
                    raise ValueError("fold_level: the layers moved from %s to %s - fold them again" % (self.device, conv.weight.device))
                _lib.call("svnet_sa_fold_f32", _ops._p(conv.weight.detach()), _ops._p(conv.bias.detach()), _ops._p(bn.weight.detach()),
                          _ops._p(bn.bias.detach()), _ops._p(bn.running_mean), _ops._p(bn.running_var), wf.shape[0], wf.shape[1],
                          float(bn.eps), _ops._p(wf), _ops._p(bf), _ops._stream())
        return self


def fold_level(convs, bns):
    """The 1x1 convolutions (Conv2d or Conv1d with a bias) and BatchNorms of one level, on a HIP device -> FoldedLevel."""
    return FoldedLevel(convs, bns)


def _launch(xyz, new_xyz, idx, idx_ld, points, level, count, count_ld, xyz_last, out, c_off, B, N, S, K, D):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_sa_fused_f32", _ops._p(xyz), _ops._p(new_xyz), _ops._p(points if D else None), _ops._p(idx), idx_ld, _ops._p(count),
                  count_ld, B, N, S, K, D, len(level.widths), level._c_widths, level._c_wf, level._c_bf, int(bool(xyz_last)), _ops._p(out),
                  int(out.shape[1]), c_off, _ops._stream())


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
    if not isinstance(level, FoldedLevel):
        raise TypeError("%s: level must be a FoldedLevel (fold_level), got %s" % (name, type(level).__name__))
    tensors, dtypes = {"xyz": xyz, "new_xyz": new_xyz}, [torch.float32, torch.float32]
    if points is not None:
        tensors["points"] = points
        dtypes.append(torch.float32)
    if out is not None:
        tensors["out"] = out
        dtypes.append(torch.float32)
    _pointset.check_tensors(name, tensors, dtypes, _WHAT)
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
    if level.c_in != 3 + D:
        raise ValueError("%s: the level takes %d input columns, xyz and points give 3 + %d" % (name, level.c_in, D))
    c_off, C = int(c_off), level.widths[-1]
    if out is not None and (out.dim() != 3 or out.shape[0] != B or out.shape[2] != S or c_off < 0 or c_off + C > out.shape[1]):
        raise ValueError("%s: out must be [B,C_total,S] with B = %d, S = %d and channels %d .. %d inside it, got %s"
                         % (name, B, S, c_off, c_off + C - 1, tuple(out.shape)))
    if out is None and c_off:
        raise ValueError("%s: c_off = %d without out" % (name, c_off))
    _ops._hip(xyz, new_xyz, idx, points, count, out)
    if level.device != xyz.device:
        raise ValueError("%s: the level is on %s, xyz on %s" % (name, level.device, xyz.device))
    if not supported(N, S, K, D, level.widths):
        raise _lib.SvnetHipError("%s: N = %d, S = %d, K = %d, D = %d, widths %s is not supported (1 <= K <= N <= %d, S >= 1, D <= 321, 1 .. %d "
                                 "layers of width 1 .. 256)" % (name, N, S, K, D, list(level.widths), _pointset.MAX_N, MAX_LAYERS))
    if out is None:
        out = torch.empty(B, C, S, dtype=torch.float32, device=xyz.device)
    _launch(xyz, new_xyz, idx, idx_ld, points, level, count, count_ld, xyz_last, out, c_off, B, N, S, K, D)
    return out


class FusedSetAbstraction:
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

    def refresh(self):
        for level in self.levels:
            level.refresh()
        return self

    def supported(self, N, D):
        """Whether clouds of N points with D attributes take the fused path here; else __call__ runs the module."""
        R, _, c_nsample, _ = _scales("FusedSetAbstraction", self.radii, self.nsamples)
        lib = _lib.lib()
        return bool(lib.svnet_fps_supported(N, self.npoint) and lib.svnet_group_msg_supported(N, self.npoint, R, c_nsample, D)
                    and all(level.c_in == 3 + D and supported(N, self.npoint, k, D, level.widths)
                            for level, k in zip(self.levels, self.nsamples)))

    @torch.no_grad()
    def __call__(self, xyz, points, start=None):
        name = "FusedSetAbstraction"
        if self.module.training:
            raise RuntimeError("%s: the module is in train mode - this is the eval-mode forward (module.eval())" % name)
        tensors, dtypes = {"xyz": xyz}, [torch.float32]
        if points is not None:
            tensors["points"] = points
            dtypes.append(torch.float32)
        if start is not None:
            tensors["start"] = start
            dtypes.append(torch.int64)
        # (the module takes views: they are made contiguous row-major below, so contiguity is not asked for here)
        _pointset.check_tensors(name, {k: t.contiguous() if isinstance(t, torch.Tensor) else t for k, t in tensors.items()}, dtypes, _WHAT)
        if xyz.dim() != 3 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
            raise ValueError("%s: xyz must be [B,3,N], got %s" % (name, tuple(xyz.shape)))
        B, N = int(xyz.shape[0]), int(xyz.shape[2])
        if points is not None and (points.dim() != 3 or points.shape[0] != B or points.shape[2] != N):
            raise ValueError("%s: points must be [B,D,N] with B = %d, N = %d, got %s" % (name, B, N, tuple(points.shape)))
        D = 0 if points is None else int(points.shape[1])
        _ops._hip(xyz, points, start)
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
