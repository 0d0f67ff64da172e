"""Fused global set-abstraction level for inference: all points of a cloud, the shared MLP and the max as two launches
(svnet_amd/csrc/sa_global.hip).

The last level of every PointNet++ encoder is a set-abstraction level with group_all: one group of all N points around centre 0.  In
eval mode it is a pure function of a cloud: concatenate coordinates and features, run two to four 1x1 convolutions with BatchNorm's
running statistics and ReLU, take the maximum over the points.  `PointNetSetAbstraction.forward`
(svnet_amd/models/utils/pointnet_util.py) makes row-major copies of xyz and points, concatenates them into [B,1,N,3+D] and writes every
layer's activation to memory; here the inputs are read channel-first as they lie and nothing leaves the compute unit but C_out floats
per cloud.  Training is out of scope, as in svnet_amd/sa_fused.py: the module stays as it is, this is an entry beside it.  The level's
widths (256 / 512 / 1024 in the classifiers) and its input (259 or 643 columns) lie outside sa_fused's limits, and one group per cloud
is too little parallelism unless a cloud is split over workgroups: a kernel of its own on the same layer engine.

    level = sa_fused.fold_level(module.mlp_convs, module.mlp_bns)              # the same fold
    out = global_mlp_max(xyz, points, level)                                   # [B,C_out,1]
    fused = FusedGlobalAbstraction(module)                                     # PointNetSetAbstraction with group_all=True
    new_xyz, new_points = fused(xyz, points)                                   # the module's eval-mode forward

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf):

    rows        row p, 0 <= p < N: h0 = [xyz[0..2, p] | points[0..D-1, p]], bit for bit: sample_and_group_all's order, coordinates
                first and not centred (the centre is 0 and nothing is subtracted).  xyz [3,N] and points [D,N] are read channel-first.
    layers      per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc if acc > 0 else +0:
                the chain of svnet_amd/sa_fused.py, on the same layer engine.  K is never split, so no value depends on how the
                kernel tiles rows, columns or clouds.
    output      out[c_off + o] = max over p of hL_p[o] into [C_total] (that is [C_total,1]); the other channels are left alone.  The
                rows of a tile past N never enter the maximum.  The workgroups of a cloud meet by an unsigned-integer maximum on
                the bit patterns (values >= +0 order as their bits; an integer maximum has no order: reproducible bits, no float
                atomics), after a small launch of the same call has set exactly these channels to +0.
    limits      1 <= N <= 32768, 0 <= D <= 1024, 1 .. 4 layers of width 1 .. 1024 (`supported`).  Inputs are assumed finite.

A workgroup takes `rows_tile(D, widths)` consecutive points of a cloud: 64, 48, 32 or 16, the most whose activations fit in LDS.
tests/sa_global_ref.py restates the contract in numpy; the results are compared as bit patterns (a -0 counted as +0).  No argument may
require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _level, _lib, _pointset
from ._level import MAX_LAYERS, fold_level

__all__ = ["global_mlp_max", "supported", "rows_tile", "FusedGlobalAbstraction"]

_WHAT = "the fused global set-abstraction level"   # in the messages of _pointset.check_tensors
MAX_D = MAX_WIDTH = 1024
_F32 = torch.float32


def rows_tile(D, widths):
    """Consecutive points one workgroup takes for this level: 64, 48, 32 or 16; 0 outside the limits on D and the widths."""
    return int(_lib.lib().svnet_sa_global_rows_tile(int(D), *_level.c_widths(widths)))


def supported(N, D, widths):
    """Whether the fused kernel takes this level (module docstring, limits)."""
    return bool(_lib.lib().svnet_sa_global_supported(int(N), int(D), *_level.c_widths(widths)))


def _launch(xyz, points, level, out, c_off, B, N, D):
    with torch.cuda.device(xyz.device):
        _lib.call("svnet_sa_global_f32", _call.p(xyz), _call.p(points if D else None), B, N, D, len(level.widths), level._c_widths, level._c_wf,
                  level._c_bf, _call.p(out), int(out.shape[1]), c_off, _call.stream())


def global_mlp_max(xyz, points, level, out=None, c_off=0):
    """xyz [B,3,N], points [B,D,N] or None - channel-first, as the module receives them - and level a FoldedLevel for 3 + D input
    columns -> out [B,C_total,1] with channels c_off .. c_off + C_out - 1 written (module docstring); out=None allocates [B,C_out,1].
    Two launches on the current stream, no host read, no workspace.  No argument may require grad."""
    name = "global_mlp_max"
    _level.check_is_level(name, level)
    _level.check_args(name, _WHAT, {"xyz": (xyz, _F32)}, {"points": (points, _F32), "out": (out, _F32)})
    B, N, D = _level.cloud_shapes(name, xyz, points)
    _level.check_c_in(name, level, 3 + D, "xyz and points give 3 + %d" % D)
    c_off = _level.check_window(name, out, c_off, level, B, 1)
    _call.hip(xyz, points, out)
    _level.check_device(name, level, "xyz", xyz)
    if not supported(N, D, level.widths):
        raise _lib.SvnetHipError("%s: N = %d, D = %d, widths %s is not supported (1 <= N <= %d, D <= %d, 1 .. %d layers of width 1 .. %d)"
                                 % (name, N, D, list(level.widths), _pointset.MAX_N, MAX_D, MAX_LAYERS, MAX_WIDTH))
    out = _level.result(out, level, B, 1, xyz.device)
    _launch(xyz, points, level, out, c_off, B, N, D)
    return out


class FusedGlobalAbstraction(_level.FusedWrapper):
    """The eval-mode forward of a PointNetSetAbstraction with group_all=True on a HIP device, with the module's signature and results:

        fused(xyz [B,3,N], points [B,D,N] or None, start=None) -> (new_xyz [B,3,1] of zeros, new_points [B,C,1])

    `start` is accepted and ignored, as in the module: nothing is sampled.  Two launches on the current stream, no host read
    (capturable), under no_grad.  The layers are folded at construction; refresh() folds them again after the module's parameters or
    running statistics changed.  A module in train mode is refused: batch statistics are not what this computes.  A level outside the
    kernel's limits (`supported`) goes through the module's own forward.  A level with group_all=False is FusedSetAbstraction's
    (svnet_amd/sa_fused.py)."""

    def __init__(self, module):
        from .models.utils.pointnet_util import PointNetSetAbstraction
        if not isinstance(module, PointNetSetAbstraction):
            raise TypeError("FusedGlobalAbstraction: needs a PointNetSetAbstraction with group_all=True, got %s" % type(module).__name__)
        if not module.group_all:
            raise ValueError("FusedGlobalAbstraction: the module has group_all=False - that level is FusedSetAbstraction's")
        self.module = module
        self.level = fold_level(module.mlp_convs, module.mlp_bns)
        self.levels, self.channels = [self.level], self.level.widths[-1]

    def supported(self, N, D):
        """Whether clouds of N points with D attributes take the fused path here; else __call__ runs the module."""
        return bool(self.level.c_in == 3 + D and supported(N, D, self.level.widths))

    @torch.no_grad()
    def __call__(self, xyz, points, start=None):
        name = self._begin(_WHAT, {"xyz": (xyz, _F32)}, {"points": (points, _F32)})
        B, N, D = _level.cloud_shapes(name, xyz, points)
        _call.hip(xyz, points)
        if not self.supported(N, D):
            return self.module(xyz, points, start=start)
        dev = xyz.device
        _level.check_device(name, self.level, "xyz", xyz)
        out = torch.empty(B, self.channels, 1, dtype=torch.float32, device=dev)
        _launch(xyz.contiguous(), None if points is None else points.contiguous(), self.level, out, 0, B, N, D)
        return torch.zeros(B, 3, 1, dtype=torch.float32, device=dev), out
