"""Fused feature-propagation level for inference: the interpolation, the skip concatenation and the shared MLP as one launch
(svnet_amd/csrc/fp_fused.hip).

In eval mode everything a feature-propagation level does behind three_nn is a pure function of one dense point: three gathered
feature columns with three weights, the point's own skip features, two to four 1x1 convolutions with BatchNorm's running statistics
and ReLU.  `PointNetFeaturePropagation.forward` (svnet_amd/models/utils/pointnet_util.py) writes the interpolated tensor, the
concatenation and every layer's activation to memory; here nothing leaves the compute unit but C_out floats per point.  Training is
out of scope, as in svnet_amd/sa_fused.py: the module stays as it is, this is an entry beside it.

    level = sa_fused.fold_level(module.mlp_convs, module.mlp_bns)              # the same fold: Conv1d [O,C,1] and BatchNorm1d
    idx, _, weight = propagate.three_nn(rows(xyz1), rows(xyz2))                # its own launch
    out = interp_mlp(idx, weight, points2, points1, level)                     # [B,C_out,N]
    fused = FusedFeaturePropagation(module)
    new_points = fused(xyz1, xyz2, points1, points2)                           # the module's eval-mode forward

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf):

    input row   of point p: h0 = [ points1[0..D1-1, p] | y[0..D2-1] ], the order of cat([points1, interpolated]); points1 bit for bit,
                y[d] = fl(fl(fl(f[d,i0] w0) + fl(f[d,i1] w1)) + fl(f[d,i2] w2)) with f = points2 [D2,S], w_j = weight[p,j] and
                i_j = idx[p,j] clamped into 0 .. S-1: three_interpolate's arithmetic word for word (svnet_amd/propagate.py), S < 3
                included, where the empty slots are index 0 with weight 0.
    layers      per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc if acc > 0 else +0:
                the chain of svnet_amd/sa_fused.py, on the same layer engine.  K is never split, so no value depends on how the
                kernel tiles rows or columns.
    output      out[c_off + o, p] = hL_p[o], channel-first into [C_total,N]; the other channels are left alone.
    limits      N >= 1, 1 <= S <= 32768, D1 >= 0, D2 >= 1, D1 + D2 <= 1536, 1 .. 4 layers of width 1 .. 256 (`supported`).  Inputs are
                assumed finite.

A workgroup takes `rows_tile(D1, D2, widths)` consecutive points of a cloud: 64, 32 or 16, the most whose activations fit in LDS.
tests/fp_fused_ref.py restates the contract in numpy; the results are compared as bit patterns (a -0 counted as +0).  No argument may
require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _level, _lib, _pointset
from ._level import MAX_LAYERS, fold_level
from .propagate import _nn_launch

__all__ = ["interp_mlp", "supported", "rows_tile", "FusedFeaturePropagation"]

_WHAT = "the fused feature-propagation level"      # in the messages of _pointset.check_tensors
MAX_C0 = 1536
_F32 = torch.float32


def rows_tile(D1, D2, widths):
    """Consecutive points one workgroup takes for this level: 64, 32 or 16; 0 outside the limits on D1, D2 and the widths."""
    return int(_lib.lib().svnet_fp_fused_rows_tile(int(D1), int(D2), *_level.c_widths(widths)))


def supported(N, S, D1, D2, widths):
    """Whether the fused kernel takes this level (module docstring, limits)."""
    return bool(_lib.lib().svnet_fp_fused_supported(int(N), int(S), int(D1), int(D2), *_level.c_widths(widths)))


def _launch(idx, weight, points2, points1, level, out, c_off, B, N, S, D1, D2):
    with torch.cuda.device(points2.device):
        _lib.call("svnet_fp_fused_f32", _call.p(idx), _call.p(weight), _call.p(points2), _call.p(points1 if D1 else None), B, N, S, D1, D2,
                  len(level.widths), level._c_widths, level._c_wf, level._c_bf, _call.p(out), int(out.shape[1]), c_off, _call.stream())


def interp_mlp(idx, weight, points2, points1, level, out=None, c_off=0):
    """idx [B,N,3] int64 and weight [B,N,3] as three_nn gives them, points2 [B,D2,S], points1 [B,D1,N] or None, level a FoldedLevel
    for D1 + D2 input columns -> out [B,C_total,N] with channels c_off .. c_off + C_out - 1 written (module docstring); out=None
    allocates [B,C_out,N].  One launch on the current stream, no host read, no workspace.  No argument may require grad."""
    name = "interp_mlp"
    _level.check_is_level(name, level)
    _level.check_args(name, _WHAT, {"points2": (points2, _F32), "idx": (idx, torch.int64), "weight": (weight, _F32)},
                      {"points1": (points1, _F32), "out": (out, _F32)})
    if points2.dim() != 3 or points2.shape[0] < 1:
        raise ValueError("%s: points2 must be [B,D2,S], got %s" % (name, tuple(points2.shape)))
    B, D2, S = (int(v) for v in points2.shape)
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[2] != 3 or tuple(weight.shape) != tuple(idx.shape):
        raise ValueError("%s: idx and weight must be [B,N,3] with B = %d, got %s and %s" % (name, B, tuple(idx.shape), tuple(weight.shape)))
    N, D1 = int(idx.shape[1]), 0
    if points1 is not None:
        if points1.dim() != 3 or points1.shape[0] != B or points1.shape[2] != N:
            raise ValueError("%s: points1 must be [B,D1,N] with B = %d, N = %d, got %s" % (name, B, N, tuple(points1.shape)))
        D1 = int(points1.shape[1])
    _level.check_c_in(name, level, D1 + D2, "points1 and points2 give %d + %d" % (D1, D2))
    c_off = _level.check_window(name, out, c_off, level, B, N, "N")
    _call.hip(points2, idx, weight, points1, out)
    _level.check_device(name, level, "points2", points2)
    if not supported(N, S, D1, D2, level.widths):
        raise _lib.SvnetHipError("%s: N = %d, S = %d, D1 = %d, D2 = %d, widths %s is not supported (N >= 1, 1 <= S <= %d, D2 >= 1, D1 + D2 <= %d, "
                                 "1 .. %d layers of width 1 .. 256)" % (name, N, S, D1, D2, list(level.widths), _pointset.MAX_N, MAX_C0, MAX_LAYERS))
    out = _level.result(out, level, B, N, points2.device)
    _launch(idx, weight, points2, points1, level, out, c_off, B, N, S, D1, D2)
    return out


class FusedFeaturePropagation(_level.FusedWrapper):
    """The eval-mode forward of a PointNetFeaturePropagation on a HIP device, with the module's signature and result:

        fused(xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] or None, points2 [B,D2,S]) -> [B,C,N]

    three_nn -> ONE fused launch, on the current stream, no host read (capturable), under no_grad.  The layers are folded at
    construction; refresh() folds them again after the module's parameters or running statistics changed.  A module in train mode is
    refused: batch statistics are not what this computes.  A level outside the kernel's limits (`supported`) goes through the module's
    own forward."""

    def __init__(self, module):
        from .models.utils.pointnet_util import PointNetFeaturePropagation
        if not isinstance(module, PointNetFeaturePropagation):
            raise TypeError("FusedFeaturePropagation: needs a PointNetFeaturePropagation, got %s" % type(module).__name__)
        self.module = module
        self.level = fold_level(module.mlp_convs, module.mlp_bns)
        self.levels, self.channels = [self.level], self.level.widths[-1]

    def supported(self, N, S, D1, D2):
        """Whether clouds of N points over S sampled ones with D1 + D2 columns take the fused path here; else __call__ runs the module."""
        return bool(self.level.c_in == D1 + D2 and _lib.lib().svnet_propagate_supported(N, S, 1) and supported(N, S, D1, D2, self.level.widths))

    @torch.no_grad()
    def __call__(self, xyz1, xyz2, points1, points2):
        name = self._begin(_WHAT, {"xyz1": (xyz1, _F32), "xyz2": (xyz2, _F32), "points2": (points2, _F32)}, {"points1": (points1, _F32)})
        B, N, S, D1, D2 = _level.cloud_pair_shapes(name, xyz1, xyz2, points1, points2)
        _call.hip(xyz1, xyz2, points1, points2)
        if not self.supported(N, S, D1, D2):
            return self.module(xyz1, xyz2, points1, points2)
        dev = xyz1.device
        _level.check_device(name, self.level, "xyz1", xyz1)
        idx = torch.empty(B, N, 3, dtype=torch.int64, device=dev)
        dist3 = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        weight = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        _nn_launch(_pointset.rows(xyz1), _pointset.rows(xyz2), B, N, S, idx, dist3, weight)
        out = torch.empty(B, self.channels, N, dtype=torch.float32, device=dev)
        _launch(idx, weight, points2.contiguous(), None if points1 is None else points1.contiguous(), self.level, out, 0, B, N, S, D1, D2)
        return out
