"""The eval-mode forward of VN_PointNet_PSEG (svnet_amd/models/vn_pointnet_partseg.py) on the fused vector-neuron kernels: the baseline
of sv_pointnet_partseg and its natural frozen teacher for train.Distiller(..., seg=True).

Every stage has a kernel in the siblings - the position level (vn_pointnet.vn_edge_cross_mean), the point layers and the transform net
(vn_tail.vn_point, vn_cloud_mean), the norm-only layer, the std tail and the per-point coordinates - but this model's global feature is
682 vector channels wide and its std_feature 682 + 682, so conv5 + bn5, the std tail and the coordinates of the local features run in
the wide envelope of svnet_amd/vn_tail.py (wide=True: the svnet_vn_*_wide_* entries).

What is new is the head.  convs1 reads [B, 9025, N] - 2.4 GB at B 32, N 2048 - of which nothing but 825 + 2046 rows differs from point
to point.  Its weight splits by column blocks:

    [0, 4108)      on [amax of out5 | l], constant over a cloud: one [B, 4108] x [4108, 256] product, added as a bias;
    [4108, 4933)   on e1234, the coordinates of out1 .. out4 in the learnt frame;
    [4933, 6979)   on e5, the coordinates of the 682 local channels;
    [6979, 9025)   on the coordinates of the cloud mean m, e[i,k](n) = m_i . z_k(n): linear in the frame z [9, N] of the point, so
                   their contribution is G[b] z[b] with G [B, 256, 9], G[o, (a,k)] = sum_i W[o, 3 i + k] m_i[a], per cloud.  These
                   2046 rows never exist per point.

The frame itself costs no launch: three unit vectors appended to out1 .. out4 make vn_std_coords write z behind e1234 (the coordinate
of the unit vector a along frame row k is z_k[a]), so the skip block and the mean block are one batched product over 834 rows with
the per-cloud weight [W_skip | G].  Training is out of scope, as in svnet_amd/vn_fused.py, and so is pooling = 'max'.

    fused = FusedVNPointNetPSeg(model)                 # an nn.Module: folded at construction; refresh(), release()
    logits = fused(x, l)                               # x [B,3,N], l [B,16] or [B,1,16] -> [B,num_part,N]; fused.last_idx: the list of this call
"""
import torch

from . import _call, _lib, _vn
from . import vn_pointnet as _vp
from . import vn_tail as _vt

__all__ = ["FusedVNPointNetPSeg"]

_WHAT = "the fused vector-neuron PointNet part-segmentation forward"


class FusedVNPointNetPSeg(_vn.EvalOnly):
    """The eval-mode forward of a VN_PointNet_PSEG on a HIP device with the module's signature, forward(x [B,3,N], l, idx=None) ->
    logits [B,num_part,N], under no_grad.  It holds the model, so ForwardStep and Distiller(seg=True) take it as they take the model.
    The steps of the fused path:

        1.    idx = knn(x, k), or the given list [B,N,k]; pos = vn_edge_cross_mean(x, idx, conv_pos) [B,21,3,N];
        2.    out1, out2, out3 = vn_point with conv1, conv2, conv3;
        3.    the transform net: vn_point with fstn.conv1 .. conv3, vn_cloud_mean, then fstn.fc1 .. fc3 through the model's own layers
              -> g [B,42,3];
        4.    out4 = vn_point(out3, conv4, cloud=g): cat((out3, net_global)) is never built;
        5.    local = the wide vn_point_norm(out4, conv5 + bn5) [B,682,3,N];
        6.    the wide vn_tail.std_tail(local, vn1, vn2, w_lin) -> m, y, h; of h [B,8184] the model reads [:, :4092], the amax half;
        7.    e1234z = vn_std_coords(cat(out1 .. out4, three unit vectors), y, w_lin) [B,834,N] in the base envelope (278 channels);
              e5 = the wide vn_std_coords(local, y, w_lin) [B,2046,N];
        8.    the head by convs1's column blocks (module docstring), then bns1, the ReLUs and convs2 .. convs4 through the model's
              own modules (model.after_convs1).

    The layers are folded at construction and convs1's weight is split into its blocks; refresh() does both again after the
    parameters or the running statistics changed.  release() frees outgrown workspaces.  Train mode is refused, and the `training`
    flag is the model's (_vn.EvalOnly).  A model with pooling = 'max' or normalize_frame = True, and a call outside any kernel's
    limits (`supported`), run model(x, l, idx=idx).  `last_idx`: the neighbour list of the last fused call."""

    @staticmethod
    def model_class():
        from .models.vn_pointnet_partseg import VN_PointNet_PSEG
        return VN_PointNet_PSEG

    def __init__(self, model):
        from .models.vn_layers import mean_pool
        super().__init__(model)
        std = model.std_feature
        self.fused = bool(model.position_level()[1] is mean_pool and model.fstn.pool is mean_pool and not std.normalize_frame)
        self.cross, self.points, self.norm, self._std_ws = None, {}, None, None
        self.last_idx = None
        self._w1, self._eye = None, {}
        if self.fused:
            self.cross = _vp.fold_vn_cross(model.conv_pos)
            wide = int(model.conv5.map_to_feat.weight.shape[0])
            stn = int(model.fstn.fc3.map_to_feat.weight.shape[0])
            layers = [("conv1", model.conv1, 0, False), ("conv2", model.conv2, 0, False), ("conv3", model.conv3, 0, False),
                      ("conv4", model.conv4, stn, False), ("vn1", std.vn1, wide, True), ("vn2", std.vn2, 0, True)]
            layers += [("fstn%d" % i, conv, 0, False) for i, conv in enumerate(model.fstn.point_layers(), 1)]
            self.points = {key: _vt.fold_vn_point(layer, cg, wide=w) for key, layer, cg, w in layers}
            self.norm = _vt.fold_vn_linear_norm(model.conv5, model.bn5, wide=True)
            self._std_ws = _vn.Workspace(self.cross.device)
            self._split_head()

    def _split_head(self):
        """convs1's weight [256, 9025, 1] as its column blocks, contiguous: (on [h | l], on e1234, on e5, on the mean's coordinates as
        [256, 682, 3 k])."""
        w = self.model.convs1.weight.detach().squeeze(-1)
        P = self.points
        pooled, skip = 6 * self.norm.O, 3 * (P["conv1"].O + P["conv2"].O + P["conv3"].O + P["conv4"].O)
        const = pooled + (int(w.shape[1]) - 2 * pooled - skip)
        a, b = const + skip, const + skip + pooled // 2
        self._w1 = (w[:, :const].contiguous(), w[:, const:a].contiguous(), w[:, a:b].contiguous(), w[:, b:].reshape(w.shape[0], -1, 3).contiguous())

    def refresh(self):
        super().refresh()
        if self.fused:
            self._split_head()
        return self

    def _folded(self):
        return ([self.cross, self.norm] if self.fused else []) + list(self.points.values())

    def supported(self, B, N, k):
        """Whether B clouds of N points with k neighbours take the fused path here; else forward runs the model."""
        if not self.fused or not 1 <= B <= _vt.MAX_B:
            return False
        P, norm = self.points, self.norm
        chain = (self.cross.O == P["conv1"].C and P["conv1"].O == P["conv2"].C and P["conv2"].O == P["conv3"].C
                 and P["conv3"].O == P["conv4"].C == P["fstn1"].C and P["fstn1"].O == P["fstn2"].C and P["fstn2"].O == P["fstn3"].C
                 and P["conv4"].O == norm.C and norm.O == P["vn1"].C == P["vn1"].Cg and P["vn1"].O == P["vn2"].C
                 and int(self.model.convs1.weight.shape[1]) == 12 * norm.O + self._labels() + self._skip())
        return bool(chain and _vp.supported_cross(N, k, self.cross.O, self.cross.Od)
                    and all(_vt.supported_point(N, f.C, f.Cg, f.O, f.Od, f.wide) for f in P.values())
                    and _vt.supported_point_norm(N, norm.C, norm.O, True)
                    and _vt.supported_point(N, P["fstn3"].O, 0, 1, 1)                      # (the cloud mean of the transform net)
                    and _vt.supported_std(N, norm.O, norm.O, P["vn2"].O, True)
                    and _vt.supported_coords(N, self._skip() // 3 + 3, P["vn2"].O)
                    and _vt.supported_coords(N, norm.O, P["vn2"].O, True))

    def _skip(self):
        P = self.points
        return 3 * (P["conv1"].O + P["conv2"].O + P["conv3"].O + P["conv4"].O)

    def _labels(self):
        from .models.vn_pointnet_partseg import LABEL_WIDTH
        return LABEL_WIDTH

    def _units(self, B, N, device):
        """The three unit vectors as channels [B,3,3,N], expanded over B and N (no memory of its own): what makes vn_std_coords write
        the frame."""
        eye = self._eye.get(device)
        if eye is None:
            eye = self._eye[device] = torch.eye(3, dtype=torch.float32, device=device)
        return eye.view(1, 3, 3, 1).expand(B, 3, 3, N)

    @torch.no_grad()
    def encode(self, x, idx):
        """Steps 1 to 7 on the kernels: x [B,3,N] contiguous, idx [B,N,k] -> the stages {name: tensor}: "pos", "out1" .. "out4",
        "fstn", "local", "m" [B,682,3], "y", "h" [B,4092], "e1234z" [B,834,N] (its last 9 rows the frame, row 3 a + k) and "e5"
        [B,2046,N]; raises outside `supported`."""
        B, _, N = (int(v) for v in x.shape)
        if not self.supported(B, N, int(idx.shape[2])):
            raise _lib.SvnetHipError("FusedVNPointNetPSeg: B = %d, N = %d, k = %d is outside the fused path (`supported`)" % (B, N, idx.shape[2]))
        P, model = self.points, self.model
        w_lin = model.std_feature.vn_lin.weight.detach()
        st = {}
        st["pos"] = _vp.vn_edge_cross_mean(x.view(B, 1, 3, N), idx, self.cross)
        st["out1"] = _vt.vn_point(st["pos"], P["conv1"])
        st["out2"] = _vt.vn_point(st["out1"], P["conv2"])
        st["out3"] = t = _vt.vn_point(st["out2"], P["conv3"])
        for key in ("fstn1", "fstn2", "fstn3"):
            t = _vt.vn_point(t, P[key])
        st["fstn"] = g = model.fstn.head(_vt.vn_cloud_mean(t)).contiguous()
        st["out4"] = _vt.vn_point(st["out3"], P["conv4"], cloud=g)
        st["local"] = local = _vt.vn_point_norm(st["out4"], self.norm)
        st["m"], st["y"], h = _vt.std_tail(local, P["vn1"], P["vn2"], w_lin, self._std_ws, wide=True)
        st["h"] = h[:, :6 * self.norm.O]
        skip = torch.cat((st["out1"], st["out2"], st["out3"], st["out4"], self._units(B, N, x.device)), dim=1)
        st["e1234z"] = _vt.vn_std_coords(skip, st["y"], w_lin)
        st["e5"] = _vt.vn_std_coords(local, st["y"], w_lin, wide=True)
        return st

    def convs1(self, st, l):
        """convs1's output [B,256,N] from the stages and l [B,16], by the weight's column blocks (module docstring)."""
        w_const, w_skip, w_local, w_mean = self._w1
        B = int(l.shape[0])
        const = torch.addmm(self.model.convs1.bias.detach(), torch.cat((st["h"], l), dim=1), w_const.t())                     # [B,256]
        G = torch.einsum("oik,bia->boak", w_mean, st["m"]).reshape(B, w_mean.shape[0], 9)
        s = torch.matmul(w_local, st["e5"])
        s.baddbmm_(torch.cat((w_skip.unsqueeze(0).expand(B, -1, -1), G), dim=2), st["e1234z"])
        return s.add_(const.unsqueeze(-1))

    @torch.no_grad()
    def forward(self, x, l, idx=None):
        name = self._begin(_WHAT, x, l=l)
        B, N = int(x.shape[0]), int(x.shape[2])
        if idx is not None and not self.is_list(idx, B, N):
            raise ValueError("%s: idx must be the position level's neighbour list [B,N,k] int64" % name)
        l2 = self.model.label(l, B)
        for key, t in (("l", l), ("idx", idx)):
            if t is not None and t.device != x.device:
                raise ValueError("%s: x on %s, %s on %s" % (name, x.device, key, t.device))
        _call.hip(x, l, idx)
        k = self.model.k if idx is None else int(idx.shape[2])
        if not self.supported(B, N, k):
            return self.model(x, l, idx=idx)
        _vn.check_model_device(name, self.cross, "x", x)
        from .models.utils.vn_util import knn
        x = x.contiguous()
        nbr = knn(x, k) if idx is None else idx.contiguous()
        self.last_idx = nbr
        return self.model.after_convs1(self.convs1(self.encode(x, nbr), l2.contiguous()))
