"""The eval-mode forward of VN_PointNet_CLS (svnet_amd/models/vn_pointnet_cls.py) on the fused vector-neuron kernels: the baseline of
sv_pointnet_cls and its natural frozen teacher for train.Distiller - and the one piece of it that no other model has, the position level.

The position level is get_graph_feature_cross -> VNLinearLeakyReLU(3 -> 21) -> mean over k.  In torch operations it writes and re-reads
[B, 3, 3, N, k] and [B, 21, 3, N, k] tensors about ten times.  It is not linear in a per-point table - x_j x x_i depends on the pair - so
vn_fused.vn_edge_mean cannot take it; but its input is one vector channel, so an edge is nine floats and the whole level is one launch
(svnet_amd/csrc/vn_cross.hip) that writes 3 O floats per point and nothing else.  Training is out of scope, as in svnet_amd/vn_fused.py,
and so is pooling = 'max'.

    folded = fold_vn_cross(layer)                      # a VNLinearLeakyReLU over 3 -> O; buffers allocated once, refresh()
    out = vn_edge_cross_mean(x, idx, folded, out=None) # x [B,1,3,N] f32, idx [B,N,k] int64 -> [B,O,3,N]
    fused = FusedVNPointNet(model)                     # an nn.Module: folded at construction; refresh(), release()
    logits = fused(x)                                  # x [B,3,N]; fused.last_idx: the neighbour list of this call

The contract of the level, for one cloud, in the words of svnet_amd/vn_fused.py (fl() is rounding to fp32, every operation rounded
once, nothing contracted but the stated fmaf; inputs are assumed finite):

    fold        W = [map_to_feat.weight | map_to_dir.weight] stacked, [O + Od, 3]; Od = O or 1 (share_nonlinearity: every o uses
                direction row 0); s, t from BatchNorm's running statistics as vn_fused has them.
    edge        (n, j), m = idx[n,j] clamped into 0 .. N-1 before any address is formed; xi = x[:,n], xj = x[:,m];
                e0[a] = fl(xj[a] - xi[a]);  e1[a] = xi[a];  e2 = xj x xi:
                e2[0] = fl(fl(xj[1] xi[2]) - fl(xj[2] xi[1])),  e2[1] = fl(fl(xj[2] xi[0]) - fl(xj[0] xi[2])),
                e2[2] = fl(fl(xj[0] xi[1]) - fl(xj[1] xi[0])).
    product     per row r of W and component a: acc = +0; for c = 0, 1, 2: acc = fmaf(e_c[a], W[r,c], acc).  p[o,a] are the feat
                rows, d[o,a] the dir rows (row 0 for every o when Od = 1).
    norm, leaky, mean   vn_fused's three rules unchanged, with the layer's slope (0.0 in this model, any value admitted).
    limits      one vector channel in, 1 <= k <= 64, k <= N <= 32768, 1 <= O <= 128, Od is O or 1, B <= 65535 (`supported_cross`).

tests/vn_pointnet_ref.py restates the contract in numpy; the kernel's results are compared with it as bit patterns (a -0 counted as
+0).  No argument may require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _lib, _pointset, _vn
from . import vn_tail as _vt

__all__ = ["fold_vn_cross", "vn_edge_cross_mean", "supported_cross", "FoldedVNCross", "FusedVNPointNet", "MAX_K", "MAX_O", "MAX_B"]

_WHAT = "the fused vector-neuron position level"   # in the messages of _pointset.check_tensors
MAX_K, MAX_O, MAX_B = 64, 128, 65535


def supported_cross(N, k, O, Od):
    """Whether the cross edge kernel takes this level (module docstring, limits)."""
    return bool(_lib.lib().svnet_vn_cross_supported(int(N), int(k), int(O), int(Od)))


class FoldedVNCross(_vn.Folded):
    """The folded form of one VNLinearLeakyReLU over 3 -> O vector channels, the three being [x_j - x_i | x_i | x_j x x_i] of a cloud
    that is one vector channel: W [O + Od, 3] | s [O] | t [O] in one buffer on the layer's device, allocated once.  refresh() and
    release() are _vn.Folded's; the level needs no workspace."""
    NAME, ENTRY = "fold_vn_cross", "svnet_vn_cross_fold_f32"

    def __init__(self, layer):
        wf, wd, _ = _vn.check_layer(self.NAME, layer, even=False)
        if wf.shape[1] != 3:
            raise ValueError("%s: the layer takes %d vector channels, the cross edge feature of one channel has 3" % (self.NAME, wf.shape[1]))
        self.place(layer)
        self.dims = self.O, self.Od = int(wf.shape[0]), int(wd.shape[0])
        if not supported_cross(1, 1, self.O, self.Od):
            raise _lib.SvnetHipError("%s: O = %d is not supported (1 <= O <= %d)" % (self.NAME, self.O, MAX_O))
        self.allocate(3 * (self.O + self.Od) + 2 * self.O)


def fold_vn_cross(layer):
    """A VNLinearLeakyReLU over 3 -> O vector channels (the position level's), on a HIP device -> FoldedVNCross."""
    return FoldedVNCross(layer)


def _launch_cross(x, idx, folded, out, B, N, k):
    with torch.cuda.device(x.device):
        _lib.call("svnet_vn_edge_cross_mean_f32", _call.p(x), _call.p(idx), _call.p(folded.folded), B, N, k, folded.O, folded.Od, folded.slope,
                  _call.p(out), _call.stream())


def vn_edge_cross_mean(x, idx, folded, out=None):
    """x [B,1,3,N] float32, idx [B,N,k] int64 and folded a FoldedVNCross over 3 -> O -> out [B,O,3,N]: the mean over the k edges of the
    layer's eval-mode forward on [x_j - x_i | x_i | x_j x x_i] (module docstring).  One launch on the current stream, no host read, no
    workspace.  Entries of idx outside 0 .. N-1 are clamped into the cloud.  No argument may require grad."""
    name = "vn_edge_cross_mean"
    B, _, N, k = _vn.check_entry(name, _WHAT, {"x": x, "idx": idx, "out": out}, folded=folded, cls=FoldedVNCross, maker="vn_pointnet.fold_vn_cross",
                                 channels=1)
    shape = (B, folded.O, 3, N)
    _vn.check_out(name, out, shape, "[B,O,3,N]", (x, idx, out), folded)
    if B > MAX_B or not supported_cross(N, k, folded.O, folded.Od):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, k = %d, O = %d is not supported (B <= %d, 1 <= k <= %d, k <= N <= %d, O <= %d)"
                                 % (name, B, N, k, folded.O, MAX_B, MAX_K, _pointset.MAX_N, MAX_O))
    if out is None:
        out = torch.empty(*shape, dtype=torch.float32, device=x.device)
    _launch_cross(x, idx, folded, out, B, N, k)
    return out


class FusedVNPointNet(_vn.EvalOnly):
    """The eval-mode forward of a VN_PointNet_CLS on a HIP device with the module's signature, forward(x [B,3,N], idx=None) -> logits,
    under no_grad.  It holds the model, so ForwardStep and Distiller take it as they take the model.  The steps of the fused path:

        1.    idx = knn(x, k), or the given list [B,N,k];
        2.    p = vn_edge_cross_mean(x, idx, conv_pos) [B,21,3,N];
        3.    x1 = vn_point(p, conv1);
        4.    the transform net: vn_point with fstn.conv1 .. conv3, vn_cloud_mean, then fstn.fc1 .. fc3 through the model's own layers
              (they act on [B,341,3], a few thousand numbers) -> g [B,21,3];
        5.    x2 = vn_point(x1, conv2, cloud=g): conv2 folded with its last 21 input channels constant over a cloud, so
              cat((x, x_global)) is never built;
        6.    local = vn_point_norm(x2, conv3 + bn3) [B,341,3,N];
        7.    vn_tail.std_tail(local, vn1, vn2, w_lin), as FusedVNTail runs it: the cloud mean m, vn1 with cloud = m, vn2, and
              vn_std_pool in the frame of vn2's output.  Of its h [B,4092] the model reads [:, :2046], the amax half; the entry also
              computes the mean half: known waste;
        8.    the head (fc1 / bn1, fc2 / dropout / bn2, fc3) through the model's layers.

    The layers are folded at construction; refresh() folds them again after the parameters or the running statistics changed;
    release() frees outgrown workspaces.  Train mode is refused, and the `training` flag is the model's (_vn.EvalOnly).  A model with
    pooling = 'max' or std_feature.normalize_frame set, and a call outside any kernel's limits (`supported`), run model(x, idx=idx).
    `last_idx`: the neighbour list of the last fused call, so that a comparison can replay it into the model."""

    @staticmethod
    def model_class():
        from .models.vn_pointnet_cls import VN_PointNet_CLS
        return VN_PointNet_CLS

    def __init__(self, model):
        from .models.vn_layers import mean_pool
        super().__init__(model)
        enc = model.feat
        std = enc.std_feature
        self.fused = bool(enc.position_level()[1] is mean_pool and enc.fstn.pool is mean_pool and not std.normalize_frame)
        self.cross, self.points, self.norm, self._std_ws = None, {}, None, None
        self.last_idx = None
        if self.fused:
            self.cross = fold_vn_cross(enc.conv_pos)
            wide = int(enc.conv3.map_to_feat.weight.shape[0])
            stn = int(enc.fstn.fc3.map_to_feat.weight.shape[0])
            layers = [("conv1", enc.conv1, 0), ("conv2", enc.conv2, stn), ("vn1", std.vn1, wide), ("vn2", std.vn2, 0)]
            layers += [("fstn%d" % i, conv, 0) for i, conv in enumerate(enc.fstn.point_layers(), 1)]
            self.points = {key: _vt.fold_vn_point(layer, cg) for key, layer, cg in layers}
            self.norm = _vt.fold_vn_linear_norm(enc.conv3, enc.bn3)
            self._std_ws = _vn.Workspace(self.cross.device)

    def _folded(self):
        return ([self.cross, self.norm] if self.fused else []) + list(self.points.values())

    def supported(self, B, N, k):
        """Whether B clouds of N points with k neighbours take the fused path here; else forward runs the model."""
        if not self.fused or not 1 <= B <= MAX_B:
            return False
        P = self.points
        chain = (self.cross.O == P["conv1"].C and P["conv1"].O == P["conv2"].C == P["fstn1"].C and P["fstn1"].O == P["fstn2"].C
                 and P["fstn2"].O == P["fstn3"].C and P["conv2"].O == self.norm.C and self.norm.O == P["vn1"].C == P["vn1"].Cg
                 and P["vn1"].O == P["vn2"].C)
        return bool(chain and supported_cross(N, k, self.cross.O, self.cross.Od)
                    and all(_vt.supported_point(N, f.C, f.Cg, f.O, f.Od) for f in P.values())
                    and _vt.supported_point_norm(N, self.norm.C, self.norm.O)
                    and _vt.supported_point(N, P["fstn3"].O, 0, 1, 1)                      # (the cloud mean of the transform net)
                    and _vt.supported_std(N, self.norm.O, self.norm.O, P["vn2"].O))

    @torch.no_grad()
    def encode(self, x, idx):
        """Steps 2 to 7 on the kernels: x [B,3,N] contiguous, idx [B,N,k] -> (h [B,2046], the stages {name: tensor}); raises outside
        `supported`."""
        B, _, N = (int(v) for v in x.shape)
        if not self.supported(B, N, int(idx.shape[2])):
            raise _lib.SvnetHipError("FusedVNPointNet: B = %d, N = %d, k = %d is outside the fused path (`supported`)" % (B, N, idx.shape[2]))
        P, enc = self.points, self.model.feat
        st = {}
        st["pos"] = vn_edge_cross_mean(x.view(B, 1, 3, N), idx, self.cross)
        st["conv1"] = x1 = _vt.vn_point(st["pos"], P["conv1"])
        t = x1
        for key in ("fstn1", "fstn2", "fstn3"):
            t = _vt.vn_point(t, P[key])
        st["fstn"] = g = enc.fstn.head(_vt.vn_cloud_mean(t)).contiguous()
        st["conv2"] = _vt.vn_point(x1, P["conv2"], cloud=g)
        st["local"] = local = _vt.vn_point_norm(st["conv2"], self.norm)
        h = _vt.std_tail(local, P["vn1"], P["vn2"], enc.std_feature.vn_lin.weight.detach(), self._std_ws)[2]
        return h[:, :6 * self.norm.O], st

    @torch.no_grad()
    def forward(self, x, idx=None):
        name = self._begin(_WHAT, x)
        B, N = int(x.shape[0]), int(x.shape[2])
        if idx is not None and not self.is_list(idx, B, N):
            raise ValueError("%s: idx must be the position level's neighbour list [B,N,k] int64" % name)
        if idx is not None and idx.device != x.device:
            raise ValueError("%s: x on %s, idx on %s" % (name, x.device, idx.device))
        _call.hip(x, idx)
        k = self.model.k if idx is None else int(idx.shape[2])
        if not self.supported(B, N, k):
            return self.model(x, idx=idx)
        _vn.check_model_device(name, self.cross, "x", x)
        from .models.utils.vn_util import knn
        x = x.contiguous()
        nbr = knn(x, k) if idx is None else idx.contiguous()
        self.last_idx = nbr
        h, _ = self.encode(x, nbr)
        return self.model.head(h)
