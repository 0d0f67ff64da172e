"""Set-abstraction and feature-propagation levels of a hierarchical point-set encoder on MI355X.

The counterpart of the reference module `models/utils/pointnet_util.py`: `PointNetSetAbstraction` (:166-207) and
`PointNetFeaturePropagation` (:270-320) with the reference's names, constructor and forward signatures, channel-first shapes and
state_dict keys (`mlp_convs.i.*`, `mlp_bns.i.*`; Conv2d / BatchNorm2d in the abstraction, Conv1d / BatchNorm1d in the propagation),
so a reference checkpoint loads with strict=True.  The helpers of that file are re-exported under their names.

The data path is the device's: farthest point sampling -> gather of the centres -> ball query -> grouping
(svnet_amd/group.py) in the abstraction, three_nn + three_interpolate (svnet_amd/propagate.py) in the propagation; the 1x1
convolution + BatchNorm + ReLU stacks and the max over a group are torch modules.  The features carry gradients: the backward of
the grouping and of the interpolation are the per-destination ordered sums of svnet_amd/csrc/pointset_grad.hip, bit-reproducible.
Coordinates are data and get no gradient.

Stated divergences from the reference, the ones the helpers have: the difference-form distance (svnet_amd/csrc/pointset.h); the
start of the sampling is an input - forward(xyz, points, start=None), the default being data.fps_start(self.seed, B, N), uploaded
once per (B, N, device) and kept; nsample > N is refused; an empty group takes point 0.  `PointNetSetAbstractionMsg` is in pointnet_msg.py, beside this file.
There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...data import farthest_point_sample, fps_start                                          # noqa: F401  (re-exported)
from ..._pointset import rows as _rows
from ...group import _cached_start, query_ball_point, sample_and_group, sample_and_group_all  # noqa: F401  (re-exported)
from ...propagate import propagate, three_interpolate, three_nn                               # noqa: F401  (re-exported)

__all__ = ["PointNetSetAbstraction", "PointNetFeaturePropagation", "farthest_point_sample", "query_ball_point", "sample_and_group",
           "sample_and_group_all", "three_nn", "three_interpolate"]


class PointNetSetAbstraction(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for width in mlp:
            self.mlp_convs.append(nn.Conv2d(last, width, 1))
            self.mlp_bns.append(nn.BatchNorm2d(width))
            last = width
        self.seed = 0                  # of the default sampling start (data.fps_start)
        self._starts = {}

    def _start(self, B, N, device):
        return _cached_start(self._starts, self.seed, B, N, device)

    def forward(self, xyz, points, start=None):
        """xyz [B,3,N], points [B,D,N] or None, start [B] int64 or None -> (new_xyz [B,3,S], new_points [B,mlp[-1],S])."""
        xyz = _rows(xyz)
        if points is not None:
            points = _rows(points)
        if self.group_all:
            new_xyz, new_points = sample_and_group_all(xyz, points)
        else:
            if start is None:
                start = self._start(int(xyz.shape[0]), int(xyz.shape[1]), xyz.device)
            new_xyz, new_points = sample_and_group(self.npoint, self.radius, self.nsample, xyz, points, start=start)
        new_points = new_points.permute(0, 3, 2, 1)                # [B,3+D,nsample,S]
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            new_points = F.relu(bn(conv(new_points)))
        return new_xyz.permute(0, 2, 1), torch.max(new_points, 2)[0]


class PointNetFeaturePropagation(nn.Module):
    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for width in mlp:
            self.mlp_convs.append(nn.Conv1d(last, width, 1))
            self.mlp_bns.append(nn.BatchNorm1d(width))
            last = width

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] or None, points2 [B,D2,S] -> [B,mlp[-1],N]: points2 interpolated from the S
        sampled points to the N points, behind points1, through the MLP."""
        new_points = propagate(_rows(xyz1), _rows(xyz2), points2.contiguous())
        if points1 is not None:
            new_points = torch.cat([points1, new_points], dim=1)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            new_points = F.relu(bn(conv(new_points)))
        return new_points
