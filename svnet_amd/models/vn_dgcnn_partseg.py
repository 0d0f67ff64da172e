"""VN_DGCNN_PSEG: the vector-neuron DGCNN for part segmentation, the equivariant full-precision baseline of SV_DGCNN_PSEG.

Takes the place of the reference module `models/vn_dgcnn_partseg.py`: the same constructor `(args, num_part)`, sub-module names and
registration order (bn8 is registered on its own and inside conv8, as the reference has it, so both key families exist), so its
state_dicts load with strict=True; composition only - the layers are in .vn_layers, the graph in .utils.vn_util.  Additions, as
VN_DGCNN_CLS has them: forward(x, l, idx=None) takes the three neighbour lists [B, N, k] int64 of the three edge levels in place of the
dynamic graphs; edge_levels() and tail(feats, l) name the two halves of the forward.  The eval-mode forward with the levels and the
vector part of the tail fused is svnet_amd.vn_pseg.FusedVNDGCNNPSeg.
"""
import torch
import torch.nn as nn

from .vn_layers import VNLinearLeakyReLU, VNStdFeature
from .vn_dgcnn_cls import POOLS
from .utils.vn_util import get_graph_feature

# Vector channels: a third of DGCNN's 64 scalar channels at every edge layer, of its 1024 at the global one.
EDGE_WIDTH = 64 // 3
GLOBAL_WIDTH = 1024 // 3
LABEL_WIDTH = 64                # conv7: the 16 object categories, one-hot
HEAD_WIDTHS = (256, 256, 128)
# conv8 reads [amax over the points of 2 GLOBAL_WIDTH channels x 3 frame coordinates | conv7(l) | 3 EDGE_WIDTH channels x 3 per point]
POOLED_WIDTH = 2 * GLOBAL_WIDTH * 3
HEAD_IN = POOLED_WIDTH + LABEL_WIDTH + 3 * EDGE_WIDTH * 3


def _conv_bn(c_in, c_out, bn):
    return nn.Sequential(nn.Conv1d(c_in, c_out, kernel_size=1, bias=False), bn, nn.LeakyReLU(negative_slope=0.2))


class VN_DGCNN_PSEG(nn.Module):
    def __init__(self, args, num_part=50):
        super().__init__()
        if args.pooling not in POOLS:
            raise ValueError("VN_DGCNN_PSEG: pooling must be 'max' or 'mean', got %r" % (args.pooling,))
        self.args, self.k = args, args.k
        for layer, width in zip((7, 8, 9, 10), (LABEL_WIDTH,) + HEAD_WIDTHS):
            setattr(self, "bn%d" % layer, nn.BatchNorm1d(width))
        # two layers per edge at the first two levels, one at the third; a level's first layer reads [x_j - x_i | x_i]
        for layer, c_in in enumerate((2, EDGE_WIDTH, 2 * EDGE_WIDTH, EDGE_WIDTH, 2 * EDGE_WIDTH), 1):
            setattr(self, "conv%d" % layer, VNLinearLeakyReLU(c_in, EDGE_WIDTH))
        for level in (1, 2, 3):
            setattr(self, "pool%d" % level, POOLS[args.pooling](EDGE_WIDTH))
        self.conv6 = VNLinearLeakyReLU(3 * EDGE_WIDTH, GLOBAL_WIDTH, dim=4, share_nonlinearity=True)
        self.std_feature = VNStdFeature(2 * GLOBAL_WIDTH, dim=4, normalize_frame=False)
        self.conv8 = _conv_bn(HEAD_IN, HEAD_WIDTHS[0], self.bn8)
        self.conv7 = _conv_bn(16, LABEL_WIDTH, self.bn7)
        self.dp1 = nn.Dropout(p=0.5)
        self.conv9 = _conv_bn(HEAD_WIDTHS[0], HEAD_WIDTHS[1], self.bn9)
        self.dp2 = nn.Dropout(p=0.5)
        self.conv10 = _conv_bn(HEAD_WIDTHS[1], HEAD_WIDTHS[2], self.bn10)
        self.conv11 = nn.Conv1d(HEAD_WIDTHS[2], num_part, kernel_size=1, bias=False)

    def edge_levels(self):
        """[((VNLinearLeakyReLU, ...), pool)] of the three edge levels, in order: the layers applied per edge, then the pool over k."""
        return [((self.conv1, self.conv2), self.pool1), ((self.conv3, self.conv4), self.pool2), ((self.conv5,), self.pool3)]

    def head(self, x):
        """conv8's output [B, 256, N] -> the per-point logits [B, num_part, N]."""
        return self.conv11(self.conv10(self.dp2(self.conv9(self.dp1(x)))))

    def tail(self, feats, l):
        """The network behind the edge levels: the three levels' outputs [B, 21, 3, N] and l [B, 16] -> logits [B, num_part, N]."""
        x123 = torch.cat(feats, dim=1)                                                  # [B, 63, 3, N]
        B, N = x123.size(0), x123.size(3)
        local = self.conv6(x123)                                                        # [B, 341, 3, N]
        both = torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)
        invariant, frame = self.std_feature(both)                                       # [B, 682, 3, N], the frame [B, 3, 3, N]
        coords = torch.einsum('bijm,bjkm->bikm', x123, frame).reshape(B, -1, N)         # the levels' features in the frame: [B, 189, N]
        pooled = invariant.reshape(B, -1, N).amax(dim=-1, keepdim=True)                 # [B, 2046, 1]
        label = self.conv7(l.view(B, -1, 1))                                            # [B, 64, 1]
        x = torch.cat((torch.cat((pooled, label), dim=1).expand(-1, -1, N), coords), dim=1)
        return self.head(self.conv8(x))

    def forward(self, x, l, idx=None):
        """x: [B, 3, N], l: [B, 16] one-hot -> logits [B, num_part, N].  idx: None, or the three levels' lists [B, N, k] int64."""
        if idx is not None and len(idx) != 3:
            raise ValueError("VN_DGCNN_PSEG: idx must hold the three levels' neighbour lists, got %d" % len(idx))
        x = x.unsqueeze(1)
        feats = []
        for i, (convs, pool) in enumerate(self.edge_levels()):
            x = get_graph_feature(x, k=self.k, idx=None if idx is None else idx[i])
            for conv in convs:
                x = conv(x)
            x = pool(x)
            feats.append(x)
        return self.tail(feats, l)
