"""VN_PointNet_PSEG: the vector-neuron PointNet for part segmentation, the equivariant full-precision baseline of SV_PointNet_PSEG.

Takes the place of the reference module `models/vn_pointnet_partseg.py`: the same constructor `(args, num_part)`, sub-module names and
registration order, so its state_dicts load with strict=True; composition only - the layers are in .vn_layers, the graph in
.utils.vn_util.  Additions, as the siblings have them: forward(x, l, idx=None) takes ONE neighbour list [B, N, k] int64 in place of the
dynamic graph of the position level, and l as [B, 16] or [B, 1, 16] (the reference squeezes axis 1); position_level(),
point_features(), invariant() and head() / after_convs1() name the stages of the forward.  Plain torch on any device, train and eval.
The eval-mode forward on the fused kernels is svnet_amd.vn_pointnet_pseg.FusedVNPointNetPSeg.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .vn_layers import STNkd, VNBatchNorm, VNLinear, VNLinearLeakyReLU, VNMaxPool, VNStdFeature, mean_pool
from .utils.vn_util import get_graph_feature_cross

# Vector channels: a third of PointNet's 64 / 128 / 512 / 2048 scalar channels.
POINT_WIDTH, MID_WIDTH, LOCAL_WIDTH, GLOBAL_WIDTH = 64 // 3, 128 // 3, 512 // 3, 2048 // 3
LABEL_WIDTH = 16                # the object categories, one-hot
HEAD_WIDTHS = (256, 256, 128)
# convs1 reads [amax over the points of 2 GLOBAL_WIDTH channels x 3 frame coordinates | l | out1..out4 in the frame | the same 2 GLOBAL_WIDTH
# channels x 3 per point]: 4092 + 16 + 825 + 4092 = 9025
POOLED_WIDTH = 2 * GLOBAL_WIDTH * 3
SKIP_WIDTH = (POINT_WIDTH + 2 * MID_WIDTH + LOCAL_WIDTH) * 3
HEAD_IN = POOLED_WIDTH + LABEL_WIDTH + SKIP_WIDTH + POOLED_WIDTH


class VN_PointNet_PSEG(nn.Module):
    def __init__(self, args, num_part=50):
        super().__init__()
        if args.pooling not in ("max", "mean"):
            raise ValueError("VN_PointNet_PSEG: pooling must be 'max' or 'mean', got %r" % (args.pooling,))
        self.args, self.k, self.num_part = args, args.k, num_part
        self.conv_pos = VNLinearLeakyReLU(3, POINT_WIDTH, dim=5, negative_slope=0.0)
        self.conv1 = VNLinearLeakyReLU(POINT_WIDTH, POINT_WIDTH, dim=4, negative_slope=0.0)
        self.conv2 = VNLinearLeakyReLU(POINT_WIDTH, MID_WIDTH, dim=4, negative_slope=0.0)
        self.conv3 = VNLinearLeakyReLU(MID_WIDTH, MID_WIDTH, dim=4, negative_slope=0.0)
        self.conv4 = VNLinearLeakyReLU(2 * MID_WIDTH, LOCAL_WIDTH, dim=4, negative_slope=0.0)
        self.conv5 = VNLinear(LOCAL_WIDTH, GLOBAL_WIDTH)
        self.bn5 = VNBatchNorm(GLOBAL_WIDTH, dim=4)
        self.std_feature = VNStdFeature(2 * GLOBAL_WIDTH, dim=4, normalize_frame=False, negative_slope=0.0)
        self.pool = VNMaxPool(POINT_WIDTH) if args.pooling == "max" else mean_pool
        self.fstn = STNkd(args, d=MID_WIDTH)
        self.convs1 = nn.Conv1d(HEAD_IN, HEAD_WIDTHS[0], 1)
        self.convs2 = nn.Conv1d(HEAD_WIDTHS[0], HEAD_WIDTHS[1], 1)
        self.convs3 = nn.Conv1d(HEAD_WIDTHS[1], HEAD_WIDTHS[2], 1)
        self.convs4 = nn.Conv1d(HEAD_WIDTHS[2], num_part, 1)
        self.bns1 = nn.BatchNorm1d(HEAD_WIDTHS[0])
        self.bns2 = nn.BatchNorm1d(HEAD_WIDTHS[1])
        self.bns3 = nn.BatchNorm1d(HEAD_WIDTHS[2])

    def position_level(self):
        """(VNLinearLeakyReLU, pool) of the level on [x_j - x_i | x_i | x_j x x_i]."""
        return self.conv_pos, self.pool

    def point_features(self, pos):
        """pos [B, 21, 3, N], the position level's output -> (out1 [B,21,3,N], out2 [B,42,3,N], out3 [B,42,3,N], the transform net's
        vectors g [B,42,3], out4 [B,170,3,N]): conv1 .. conv3, then conv4 on [out3 | g appended to every point]."""
        out1 = self.conv1(pos)
        out2 = self.conv2(out1)
        out3 = self.conv3(out2)
        g = self.fstn(out3)
        out4 = self.conv4(torch.cat((out3, g.unsqueeze(-1).expand(-1, -1, -1, out3.size(-1))), dim=1))
        return out1, out2, out3, g, out4

    def invariant(self, out4):
        """out4 [B, 170, 3, N] -> (out5 [B, 4092, N]: the coordinates of [local | its mean over the points] in the learnt frame,
        local = bn5(conv5(out4)); the frame [B, 3, 3, N])."""
        local = self.bn5(self.conv5(out4))
        both = torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)
        out5, frame = self.std_feature(both)
        return out5.reshape(out5.size(0), -1, out5.size(-1)), frame

    def after_convs1(self, s):
        """convs1's output [B, 256, N] -> the per-point logits [B, num_part, N]."""
        net = F.relu(self.bns1(s))
        net = F.relu(self.bns2(self.convs2(net)))
        net = F.relu(self.bns3(self.convs3(net)))
        return self.convs4(net)

    def head(self, concat):
        """What stands in front of convs1, [B, 9025, N] = [amax of out5 | l, both over every point | out1..out4 in the frame | out5] ->
        the per-point logits [B, num_part, N]."""
        return self.after_convs1(self.convs1(concat))

    @staticmethod
    def label(l, B):
        """l as [B, 16]: [B, 16] itself or the reference's [B, 1, 16]."""
        if l.dim() == 3 and l.size(1) == 1:
            l = l.squeeze(1)
        if l.dim() != 2 or l.size(0) != B or l.size(1) != LABEL_WIDTH:
            raise ValueError("VN_PointNet_PSEG: l must be [B,%d] or [B,1,%d] with B = %d, got %s" % (LABEL_WIDTH, LABEL_WIDTH, B, tuple(l.shape)))
        return l

    def forward(self, x, l, idx=None):
        """x: [B, 3, N], l: [B, 16] (or [B, 1, 16]) one-hot -> logits [B, num_part, N].  idx: None, or the neighbour list [B, N, k]
        int64 of the position level."""
        if idx is not None and (not isinstance(idx, torch.Tensor) or idx.dim() != 3):
            raise ValueError("VN_PointNet_PSEG: idx must be one neighbour list [B,N,k], got %s"
                             % (tuple(idx.shape) if isinstance(idx, torch.Tensor) else type(idx).__name__))
        B, _, N = x.size()
        l = self.label(l, B)
        conv_pos, pool = self.position_level()
        pos = pool(conv_pos(get_graph_feature_cross(x.unsqueeze(1), k=self.k, idx=idx)))
        out1, out2, out3, _, out4 = self.point_features(pos)
        out5, frame = self.invariant(out4)
        pooled = torch.cat((out5.max(dim=-1)[0], l), dim=1)                             # [B, 4108]
        out1234 = torch.einsum('bijm,bjkm->bikm', torch.cat((out1, out2, out3, out4), dim=1), frame).reshape(B, -1, N)
        return self.head(torch.cat((pooled.unsqueeze(-1).expand(-1, -1, N), out1234, out5), dim=1))
