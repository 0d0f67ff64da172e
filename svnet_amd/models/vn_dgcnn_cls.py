"""VN_DGCNN_CLS: the vector-neuron DGCNN classifier, the equivariant full-precision baseline of SV_DGCNN_CLS.

Takes the place of the reference module `models/vn_dgcnn_cls.py`: the same constructor `(args, num_class)`, sub-module names and
registration order, so its state_dicts load with strict=True; composition only - the layers are in .vn_layers, the graph in
.utils.vn_util.  One addition: forward(x, idx=None) takes the four neighbour lists [B, N, k] int64 of the four edge levels in place of
the dynamic graphs; with them the forward is a continuous function of its inputs, plain torch on any device.  The eval-mode forward
with the four edge levels fused is svnet_amd.vn_fused.FusedVNDGCNN.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .vn_layers import VNLinearLeakyReLU, VNMaxPool, VNStdFeature, mean_pool
from .utils.vn_util import get_graph_feature

# Vector channels: a third of DGCNN's 64 / 64 / 128 / 256 scalar channels at the four edge levels, of its 1024 at the global one.
EDGE_WIDTHS = (21, 21, 42, 85)
GLOBAL_WIDTH = 341
HEAD_WIDTHS = (512, 256)
POOLS = {"max": VNMaxPool, "mean": lambda width: mean_pool}


class VN_DGCNN_CLS(nn.Module):
    def __init__(self, args, num_class=40):
        super().__init__()
        if args.pooling not in POOLS:
            raise ValueError("VN_DGCNN_CLS: pooling must be 'max' or 'mean', got %r" % (args.pooling,))
        self.args, self.k = args, args.k
        # conv1 .. conv4 on [x_j - x_i | x_i]: twice the channels of the level before, the cloud itself being one vector channel
        for level, (c_in, c_out) in enumerate(zip((1,) + EDGE_WIDTHS, EDGE_WIDTHS), 1):
            setattr(self, "conv%d" % level, VNLinearLeakyReLU(2 * c_in, c_out))
        self.conv5 = VNLinearLeakyReLU(sum(EDGE_WIDTHS), GLOBAL_WIDTH, dim=4, share_nonlinearity=True)
        self.std_feature = VNStdFeature(2 * GLOBAL_WIDTH, dim=4, normalize_frame=False)
        # the head reads [max | mean] over the points of 2 GLOBAL_WIDTH channels x 3 frame coordinates
        widths = (2 * 3 * 2 * GLOBAL_WIDTH,) + HEAD_WIDTHS
        for layer, (c_in, c_out) in enumerate(zip(widths, HEAD_WIDTHS), 1):
            setattr(self, "linear%d" % layer, nn.Linear(c_in, c_out))
            setattr(self, "bn%d" % layer, nn.BatchNorm1d(c_out))
            setattr(self, "dp%d" % layer, nn.Dropout(p=0.5))
        self.linear3 = nn.Linear(HEAD_WIDTHS[-1], num_class)
        for level, width in enumerate(EDGE_WIDTHS, 1):                 # (a VNMaxPool has parameters: registered last, as the reference's)
            setattr(self, "pool%d" % level, POOLS[args.pooling](width))

    def edge_levels(self):
        """[(VNLinearLeakyReLU, pool)] of the four edge levels, in order."""
        return [(getattr(self, "conv%d" % i), getattr(self, "pool%d" % i)) for i in range(1, len(EDGE_WIDTHS) + 1)]

    def tail(self, feats):
        """The network behind the edge levels: the four levels' outputs [B, C_i, 3, N] -> logits [B, num_class]."""
        local = self.conv5(torch.cat(feats, dim=1))                                     # [B, 341, 3, N]
        both = torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)
        invariant = self.std_feature(both)[0].flatten(1, 2)                             # [B, 682 * 3, N]: coordinates in the learnt frame
        h = torch.cat((invariant.amax(dim=-1), invariant.mean(dim=-1)), dim=1)
        for layer in (1, 2):
            linear, bn, drop = (getattr(self, "%s%d" % (name, layer)) for name in ("linear", "bn", "dp"))
            h = drop(F.leaky_relu(bn(linear(h)), negative_slope=0.2))
        return self.linear3(h)

    def forward(self, x, idx=None):
        """x: [B, 3, N] -> logits [B, num_class].  idx: None, or the four levels' neighbour lists [B, N, k] int64."""
        if idx is not None and len(idx) != 4:
            raise ValueError("VN_DGCNN_CLS: idx must hold the four levels' neighbour lists, got %d" % len(idx))
        x = x.unsqueeze(1)
        feats = []
        for i, (conv, pool) in enumerate(self.edge_levels()):
            x = pool(conv(get_graph_feature(x, k=self.k, idx=None if idx is None else idx[i])))
            feats.append(x)
        return self.tail(feats)
