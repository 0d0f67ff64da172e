"""VN_PointNet_CLS: the vector-neuron PointNet classifier, the equivariant full-precision baseline of SV_PointNet_CLS.

Takes the place of the reference module `models/vn_pointnet_cls.py`: the same constructors `PointNetEncoder(args)` and
`VN_PointNet_CLS(args, num_class)`, sub-module names and registration order, so its state_dicts load with strict=True; composition
only - the layers are in .vn_layers, the graph in .utils.vn_util.  One addition, as in VN_DGCNN_CLS: forward(x, idx=None) takes ONE
neighbour list [B, N, k] int64 in place of the dynamic graph of the position level; with it the forward is a continuous function of
its inputs, plain torch on any device.  The eval-mode forward on the fused kernels is svnet_amd.vn_pointnet.FusedVNPointNet.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .vn_layers import STNkd, VNBatchNorm, VNLinear, VNLinearLeakyReLU, VNMaxPool, VNStdFeature, mean_pool
from .utils.vn_util import get_graph_feature_cross

# Vector channels: a third of PointNet's 64 / 128 / 1024 scalar channels.
POINT_WIDTH, MID_WIDTH, GLOBAL_WIDTH = 64 // 3, 128 // 3, 1024 // 3
HEAD_WIDTHS = (512, 256)


class PointNetEncoder(nn.Module):
    """x [B, 3, N] -> h [B, 6 GLOBAL_WIDTH]: the maximum over the points of [local | its mean over the points] in the learnt frame."""

    def __init__(self, args):
        super().__init__()
        if args.pooling not in ("max", "mean"):
            raise ValueError("PointNetEncoder: pooling must be 'max' or 'mean', got %r" % (args.pooling,))
        self.args, self.k = args, args.k
        self.conv_pos = VNLinearLeakyReLU(3, POINT_WIDTH, dim=5, negative_slope=0.0)
        self.conv1 = VNLinearLeakyReLU(POINT_WIDTH, POINT_WIDTH, dim=4, negative_slope=0.0)
        self.conv2 = VNLinearLeakyReLU(2 * POINT_WIDTH, MID_WIDTH, dim=4, negative_slope=0.0)
        self.conv3 = VNLinear(MID_WIDTH, GLOBAL_WIDTH)
        self.bn3 = VNBatchNorm(GLOBAL_WIDTH, dim=4)
        self.std_feature = VNStdFeature(2 * GLOBAL_WIDTH, dim=4, normalize_frame=False, negative_slope=0.0)
        self.pool = VNMaxPool(POINT_WIDTH) if args.pooling == "max" else mean_pool
        self.fstn = STNkd(args, d=POINT_WIDTH)

    def position_level(self):
        """(VNLinearLeakyReLU, pool) of the level on [x_j - x_i | x_i | x_j x x_i]."""
        return self.conv_pos, self.pool

    def local_feature(self, x):
        """x [B, 21, 3, N], the position level's output -> local [B, 341, 3, N]: conv1, the transform net's vectors appended to every
        point, conv2 and the norm-only conv3 + bn3."""
        x = self.conv1(x)
        x_global = self.fstn(x).unsqueeze(-1).expand(-1, -1, -1, x.size(-1))
        return self.bn3(self.conv3(self.conv2(torch.cat((x, x_global), dim=1))))

    def pooled(self, local):
        """local [B, 341, 3, N] -> h [B, 2046]: column 3 i + k is coordinate k of channel i of [local | its mean], maximum over the points."""
        both = torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)
        return self.std_feature(both)[0].flatten(1, 2).max(dim=-1)[0]

    def forward(self, x, idx=None):
        """x: [B, 3, N] -> [B, 2046].  idx: None, or the position level's neighbour list [B, N, k] int64."""
        conv_pos, pool = self.position_level()
        x = pool(conv_pos(get_graph_feature_cross(x.unsqueeze(1), k=self.k, idx=idx)))
        return self.pooled(self.local_feature(x))


class VN_PointNet_CLS(nn.Module):
    def __init__(self, args, num_class=40):
        super().__init__()
        self.args = args
        self.feat = PointNetEncoder(args)
        self.fc1 = nn.Linear(6 * GLOBAL_WIDTH, HEAD_WIDTHS[0])
        self.fc2 = nn.Linear(HEAD_WIDTHS[0], HEAD_WIDTHS[1])
        self.fc3 = nn.Linear(HEAD_WIDTHS[1], num_class)
        self.dropout = nn.Dropout(p=0.4)
        self.bn1 = nn.BatchNorm1d(HEAD_WIDTHS[0])
        self.bn2 = nn.BatchNorm1d(HEAD_WIDTHS[1])
        self.relu = nn.ReLU()

    @property
    def k(self):
        return self.feat.k

    def head(self, h):
        """h [B, 2046], the encoder's output -> logits [B, num_class]."""
        h = F.relu(self.bn1(self.fc1(h)))
        h = F.relu(self.bn2(self.dropout(self.fc2(h))))
        return self.fc3(h)

    def forward(self, x, idx=None):
        """x: [B, 3, N] -> logits [B, num_class].  idx: None, or the neighbour list [B, N, k] int64 of the position level."""
        if idx is not None and (not isinstance(idx, torch.Tensor) or idx.dim() != 3):
            raise ValueError("VN_PointNet_CLS: idx must be one neighbour list [B,N,k], got %s"
                             % (tuple(idx.shape) if isinstance(idx, torch.Tensor) else type(idx).__name__))
        return self.head(self.feat(x, idx=idx))
