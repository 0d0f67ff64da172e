"""The eval-mode forward of VN_DGCNN_PSEG (svnet_amd/models/vn_dgcnn_partseg.py) on the fused vector-neuron kernels: the part-segmentation
baseline, and the natural frozen teacher of train.Distiller(..., seg=True).

Two of the model's three edge levels apply two VNLinearLeakyReLU layers per edge in front of the mean over the neighbours.  In torch
operations at B 32, N 2048, k 40 they work on [32, 21..42, 3, 2048, 40] tensors, 0.66 to 1.3 GB each and more than a dozen of them; here
a level is the tables of its first layer and one edge pass that keeps the first layer's outputs on the chip (vn_fused.vn_edge2_mean).
Behind the levels the learnt frame is applied to the per-point features, not only pooled: vn_tail.vn_std_coords.  The head's per-point
convolutions stay torch, but the [B, 2299, N] input of conv8 is never built: 2110 of its channels are constant over a cloud,

    conv8 = W8[:, 2110:] e123 + (W8[:, :2110] [h | conv7(l)])[:, :, None],

one small product per cloud and one [256, 189] product per point.  Training is out of scope, as in svnet_amd/vn_fused.py, and so is
pooling = 'max'.

    fused = FusedVNDGCNNPSeg(model)                    # an nn.Module: folded at construction; refresh(), release()
    logits = fused(x, l)                               # x [B,3,N], l [B,16] -> [B,num_part,N]; fused.last_idx: the three lists of this call
"""
import torch

from . import _vn
from . import vn_fused as _vf
from . import vn_tail as _vt

__all__ = ["FusedVNDGCNNPSeg"]

_WHAT = "the fused vector-neuron part-segmentation forward"


class FusedVNDGCNNPSeg(_vn.EvalOnly):
    """The eval-mode forward of a VN_DGCNN_PSEG on a HIP device with the module's signature, forward(x [B,3,N], l [B,16], idx=None) ->
    logits [B,num_part,N], under no_grad.  It holds the model, so ForwardStep and Distiller(seg=True) take it as they take the model.
    The steps of the fused path:

        1-3.  per level knn (or the given list), then the tables of its first layer and the edge pass: vn_edge2_mean for (conv1, conv2)
              and (conv3, conv4), vn_edge_mean for conv5 -> x1, x2, x3 [B,21,3,N];
        4.    x123 = cat(x1, x2, x3) (the edge entries have no channel window to write into one buffer);
        5.    local = vn_point(x123, conv6);
        6-8.  vn_tail.std_tail(local, vn1, vn2, w_lin): the cloud mean m, vn1 with cloud = m, vn2 -> y, and vn_std_pool in y's frame.
              Of its h the model reads [:, :3 * 682], the amax half; the entry also computes the mean half: a known small cost (the
              sums ride on the loop that finds the maxima);
        9.    e123 = vn_std_coords(x123, y, w_lin) [B,189,N];
        10.   the head in torch without the [B,2299,N] tensor (module docstring), then bn8, the leaky rule and conv9 .. conv11 through
              the model's own modules.

    The layers are folded at construction, and conv8's weight is split into its two column blocks; refresh() does both again after the
    parameters or the running statistics changed.  release() frees outgrown workspaces.  Train mode is refused, and the `training`
    flag is the model's (_vn.EvalOnly).  A model with pooling = 'max' or normalize_frame = True, and a call outside the kernels'
    limits (`supported`), run model(x, l, idx=idx).  `last_idx`: the three neighbour lists of the last fused call."""

    @staticmethod
    def model_class():
        from .models.vn_dgcnn_partseg import VN_DGCNN_PSEG
        return VN_DGCNN_PSEG

    def __init__(self, model):
        from .models.vn_layers import mean_pool
        super().__init__(model)
        std = model.std_feature
        self.fused = bool(all(pool is mean_pool for _, pool in model.edge_levels()) and not std.normalize_frame)
        self.levels, self.points, self._std_ws = [], [], None
        self.last_idx = None
        self._w8 = None
        if self.fused:
            self.levels = [(_vf.fold_vn_layer(convs[0]),) + tuple(_vt.fold_vn_point(c) for c in convs[1:]) for convs, _ in model.edge_levels()]
            wide = int(model.conv6.map_to_feat.weight.shape[0])
            self.points = [_vt.fold_vn_point(model.conv6), _vt.fold_vn_point(std.vn1, wide), _vt.fold_vn_point(std.vn2)]
            self._std_ws = _vn.Workspace(self.points[0].device)
            self._split_head()

    def _split_head(self):
        """conv8's weight [256, 2299, 1] as its two column blocks, contiguous: the cloud's constant channels and the per-point ones."""
        w = self.model.conv8[0].weight.detach().squeeze(-1)
        const = 6 * self.points[0].O + int(self.model.conv7[0].weight.shape[0])
        self._w8 = (w[:, :const].contiguous(), w[:, const:].contiguous())

    def refresh(self):
        super().refresh()
        if self.fused:
            self._split_head()
        return self

    def _folded(self):
        return [f for level in self.levels for f in level] + list(self.points)

    def supported(self, B, N, k):
        """Whether B clouds of N points with k neighbours take the fused path here; else forward runs the model."""
        if not self.fused or not 1 <= B <= _vt.MAX_B:
            return False
        for level in self.levels:
            f1 = level[0]
            if len(level) == 2:
                if level[1].C != f1.O or not _vf.supported2(N, k, f1.C, f1.O, f1.Od, level[1].O, level[1].Od):
                    return False
            elif not _vf.supported(N, k, f1.C, f1.O, f1.Od):
                return False
        conv6, vn1, vn2 = self.points
        x123 = sum(level[-1].O for level in self.levels)
        return bool(conv6.C == x123 and all(_vt.supported_point(N, f.C, f.Cg, f.O, f.Od) for f in self.points)
                    and _vt.supported_std(N, conv6.O, conv6.O, vn2.O) and _vt.supported_coords(N, x123, vn2.O))

    @staticmethod
    def _launch_level(h, nbr, level, out, B, N, k):
        """A level's launches: the tables of its first layer, then the two-layer edge pass or, for a single layer, vn_edge_mean's."""
        if len(level) == 2:
            _vf._launch2(h, nbr, level[0], level[1], out, B, N, k)
        else:
            _vf._launch(h, nbr, level[0], out, B, N, k)

    @torch.no_grad()
    def forward(self, x, l, idx=None):
        name = self._begin(_WHAT, x, l=l)
        model = self.model
        if l.dim() != 2 or l.shape[0] != x.shape[0] or l.shape[1] != model.conv7[0].weight.shape[1]:
            raise ValueError("%s: l must be [B,%d] with B = %d, got %s" % (name, model.conv7[0].weight.shape[1], x.shape[0], tuple(l.shape)))
        B, N, ks = self._lists(name, x, idx, 3, others=(l,))
        if not all(self.supported(B, N, k) for k in ks):
            return model(x, l, idx=idx)
        _vn.check_model_device(name, self.points[0], "x", x)
        feats = self._edge_levels(x, idx, ks, [(level, level[-1].O) for level in self.levels], self._launch_level)
        conv6, vn1, vn2 = self.points
        w_lin = model.std_feature.vn_lin.weight.detach()
        x123 = torch.cat(feats, dim=1)
        _, y, pooled = _vt.std_tail(_vt.vn_point(x123, conv6), vn1, vn2, w_lin, self._std_ws)
        pooled = pooled[:, :6 * conv6.O]
        e123 = _vt.vn_std_coords(x123, y, w_lin)
        # the head: conv8 on [pooled | conv7(l)] expanded over the points and e123, as two products
        w_const, w_point = self._w8
        const = torch.cat((pooled, model.conv7(l.contiguous().view(B, -1, 1)).squeeze(-1)), dim=1) @ w_const.t()      # [B, 256]
        h8 = torch.matmul(w_point, e123).add_(const.unsqueeze(-1))
        for layer in list(model.conv8)[1:]:
            h8 = layer(h8)
        return model.head(h8)
