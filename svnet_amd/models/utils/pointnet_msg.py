"""The multi-scale set-abstraction level of a hierarchical point-set encoder on MI355X.

The counterpart of `PointNetSetAbstractionMsg` of the reference module `models/utils/pointnet_util.py` (:210-267), the encoder level
of the PointNet++ MSG classifiers and part-segmentation nets, with the reference's name, constructor signature, channel-first shapes
and state_dict keys (`conv_blocks.i.j.*`, `bn_blocks.i.j.*`, Conv2d / BatchNorm2d), so a reference checkpoint loads with strict=True.
It lives beside svnet_amd/models/utils/pointnet_util.py, which holds the single-scale level and the propagation and is left as it is.

The data path is the device's: farthest point sampling -> gather of the centres -> ONE ball-query pass for all radii -> ONE grouping
launch (svnet_amd/group.py, "Multi-scale grouping"; svnet_amd/csrc/group.hip); the 1x1 convolution + BatchNorm + ReLU stacks, the
max over a group and the cat of the scales on the channel axis are torch modules.  The attributes carry gradients (the ordered sums of
group_points_msg_backward, bit-reproducible); coordinates are data and get no gradient.

Stated divergences from the reference, the ones pointnet_util.py has: the difference-form distance; the start of the sampling is an
input - forward(xyz, points, start=None), the default being data.fps_start(self.seed, B, N), uploaded once per (B, N, device) and
kept; nsample > N is refused; an empty group takes point 0; at most four scales.  There is no CPU fallback.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..._pointset import rows as _rows
from ...group import _cached_start, query_ball_point_msg, sample_and_group_msg                 # noqa: F401  (re-exported)

__all__ = ["PointNetSetAbstractionMsg", "query_ball_point_msg", "sample_and_group_msg"]


class PointNetSetAbstractionMsg(nn.Module):
    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for mlp in mlp_list:
            convs, bns, last = nn.ModuleList(), nn.ModuleList(), in_channel + 3
            for width in mlp:
                convs.append(nn.Conv2d(last, width, 1))
                bns.append(nn.BatchNorm2d(width))
                last = width
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)
        self.seed = 0                  # of the default sampling start (data.fps_start)
        self._starts = {}

    def _start(self, B, N, device):
        return _cached_start(self._starts, self.seed, B, N, device)

    def forward(self, xyz, points, start=None):
        """xyz [B,3,N], points [B,D,N] or None, start [B] int64 or None -> (new_xyz [B,3,S], new_points [B,sum of mlp[-1],S]): the
        scales' results behind each other on the channel axis."""
        xyz = _rows(xyz)
        if points is not None:
            points = _rows(points)
        if start is None:
            start = self._start(int(xyz.shape[0]), int(xyz.shape[1]), xyz.device)
        new_xyz, grouped = sample_and_group_msg(self.npoint, self.radius_list, self.nsample_list, xyz, points, start=start)
        scales = []
        for new_points, convs, bns in zip(grouped, self.conv_blocks, self.bn_blocks):
            new_points = new_points.permute(0, 3, 2, 1)            # [B,D+3,nsample_i,S]
            for conv, bn in zip(convs, bns):
                new_points = F.relu(bn(conv(new_points)))
            scales.append(torch.max(new_points, 2)[0])
        return new_xyz.permute(0, 2, 1), torch.cat(scales, dim=1)
