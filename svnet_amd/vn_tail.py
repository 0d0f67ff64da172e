"""Fused vector-neuron tail for inference: conv5, the cloud mean, VNStdFeature and the [amax | mean] pool of VN_DGCNN_CLS.tail as
per-point kernels (svnet_amd/csrc/vn_tail.hip), and the eval-mode tail of the classifier on top of them.

In torch operations the tail works on [B, 341, 3, N] and [B, 682, 3, N] tensors and writes and re-reads more than twenty of them.
Here a VNLinearLeakyReLU is one launch that writes its 3 O floats per point and nothing else, the mean over the points is one launch,
and VNStdFeature's frame, its einsum and the two pools are one launch and a small finish that never write the [B, 2046, N] tensor.
`both = [local | mean_N(local) expanded]` is never built: half of vn1's K axis is constant over a cloud,

    W both = W[:, :341] local + W[:, 341:] m,

so the second term is one small product per cloud (the cloud term) and the chain of a point starts from it.  Training is out of
scope, as in svnet_amd/vn_fused.py: the modules stay as they are, this is an entry beside them.

    folded = fold_vn_point(layer, cloud_channels=0)    # a VNLinearLeakyReLU over C + Cg -> O; buffers allocated once, refresh()
    out = vn_point(x, folded, cloud=None, out=None)    # x [B,C,3,N], cloud [B,Cg,3] -> [B,O,3,N]
    folded = fold_vn_linear_norm(linear, batchnorm)    # a VNLinear then a VNBatchNorm, no leaky rule, C -> O
    out = vn_point_norm(x, folded, out=None)           # x [B,C,3,N] -> [B,O,3,N]
    m = vn_cloud_mean(x, out=None)                     # x [B,C,3,N] -> [B,C,3]
    h = vn_std_pool(x, y, w_lin, cloud=None, out=None) # x [B,C,3,N], y [B,Cy,3,N], w_lin [3,Cy], cloud [B,Cg,3] -> [B, 6 (C + Cg)]
    e = vn_std_coords(x, y, w_lin, out=None)           # the same coordinates per point, unpooled -> [B, 3 C, N] (VN_DGCNN_PSEG's head)
    tail = FusedVNTail(model)                          # the four levels' outputs -> logits; vn_fused.FusedVNDGCNN(model, tail=True)

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf;
EPS = fl(1e-6); inputs are assumed finite):

    fold        W_f = map_to_feat.weight [O, C + Cg], W_d = map_to_dir.weight [Od, C + Cg], Od = O or 1 (share_nonlinearity: every o
                uses direction row 0); W = [W_f | W_d] stacked.  s, t from BatchNorm's running statistics as vn_fused has them:
                invstd = fl(1 / fl(sqrt(fl(var + eps)))), s = fl(gamma invstd), t = fl(beta - fl(mean s)).
    cloud term  per row r of W and component a: u = +0; for c ascending over Cg: u = fmaf(g[c,a], W[r, C + c], u).
    point term  per (n, a) and row r: acc = u[r,a]; for c ascending over C: acc = fmaf(x[c,a,n], W[r,c], acc).  K is never split.
                p[o,a] are the W_f rows, d[od,a] the W_d rows.
    norm, leaky the edge level's two rules, stated in svnet_amd/vn_fused.py, on p[o,:], d[o,:], s[o] and t[o]: out[o,a,n] = y[a].
    norm only   (vn_point_norm) the point term with u = +0 and no direction rows, then the norm rule alone: q, r, g as stated there,
                out[o,a,n] = fl(p[a] g).  The same kernel with its epilogue exchanged; 1 <= C, O <= 512 (`supported_point_norm`).
    cloud mean  run j holds n in [64 j, min(N, 64 j + 64)); a run's sum is n-ascending plain additions from +0;
                m = fl((the runs' sums added j-ascending from +0) / fl(N)).  The order is the contract's, not the tiling's.
    std-pool    frame rows z[k][a](n) = +0, then fmaf(y[c,a,n], w_lin[k,c], z) for c ascending over Cy; with v_i = x[i,:,n] for i < C
                and g[i-C,:] otherwise, e[i,k](n) = fmaf(v_i[2], z[k][2], fmaf(v_i[1], z[k][1], fl(v_i[0] z[k][0])));  with I = C + Cg,
                h[3 i + k] = max over n of e, h[3 I + 3 i + k] = the mean of e under the cloud-mean rule.
    limits      1 <= N <= 32768, 1 <= C <= 512, 0 <= Cg <= 512, 1 <= O <= 512, Od is O or 1, 1 <= Cy <= 512, B <= 65535
                (`supported_point`, `supported_std`).  With wide=True - on the folds, which hand it to vn_point and vn_point_norm, and on
                vn_cloud_mean, vn_std_pool, vn_std_coords and std_tail - 768 stands for 512 throughout (MAX_C_WIDE, MAX_O_WIDE; the
                `supported_*_wide` forms): the svnet_vn_*_wide_* entries, the same kernels and the same contract.  VN_PointNet_PSEG's
                682-wide std_feature needs it; nothing takes it unasked.

The module's order of the norm and leaky arithmetic differs from the contract's in rounding only.
tests/vn_tail_ref.py restates the contract in numpy; the kernels' results are compared with it as bit patterns (a -0 counted as +0).
No argument may require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _lib, _pointset, _vn

__all__ = ["fold_vn_point", "vn_point", "vn_cloud_mean", "vn_std_pool", "vn_std_coords", "supported_point", "supported_std", "supported_coords",
           "FoldedVNPoint", "FusedVNTail", "fold_vn_linear_norm", "vn_point_norm", "supported_point_norm", "FoldedVNPointNorm",
           "MAX_C", "MAX_O", "MAX_B", "MAX_C_WIDE", "MAX_O_WIDE", "supported_point_wide", "supported_point_norm_wide", "supported_std_wide",
           "supported_coords_wide"]

_WHAT = "the fused vector-neuron tail"   # in the messages of _pointset.check_tensors
MAX_C, MAX_O, MAX_B = 512, 512, 65535
MAX_C_WIDE, MAX_O_WIDE = 768, 768
_F32 = torch.float32


def _entry(stem, rest, wide):
    """The C entry of a stage in the envelope asked for: svnet_vn_<stem>[_wide]_<rest> (include/svnet_hip.h, the naming rule)."""
    return "svnet_vn_%s%s_%s" % (stem, "_wide" if wide else "", rest)


def _widest(wide):
    """(the widest C, the widest O) of the envelope in force, for the messages."""
    return (MAX_C_WIDE, MAX_O_WIDE) if wide else (MAX_C, MAX_O)


def _ask(stem, wide, *dims):
    return bool(getattr(_lib.lib(), _entry(stem, "supported", wide))(*(int(d) for d in dims)))


def supported_point(N, C, Cg, O, Od, wide=False):
    """Whether the point-level kernel takes this layer (module docstring, limits)."""
    return _ask("point", wide, N, C, Cg, O, Od)


def supported_std(N, C, Cg, Cy, wide=False):
    """Whether the standardise-and-pool kernel takes these widths (module docstring, limits)."""
    return _ask("std_pool", wide, N, C, Cg, Cy)


def supported_point_wide(N, C, Cg, O, Od):
    """supported_point in the wide envelope."""
    return supported_point(N, C, Cg, O, Od, wide=True)


def supported_std_wide(N, C, Cg, Cy):
    """supported_std in the wide envelope."""
    return supported_std(N, C, Cg, Cy, wide=True)


_Workspace = _vn.Workspace     # (vn_std_pool takes one as its `workspace`)


class FoldedVNPoint(_vn.Folded):
    """The folded form of one VNLinearLeakyReLU over C + Cg -> O vector channels whose last Cg input channels are constant over a
    cloud: WT [C + Cg, O + Od] | s [O] | t [O] in one buffer on the layer's device, allocated once, and the workspace of the cloud
    term, which grows to the largest B seen and is then reused (`workspace`: the current one).  refresh() and release() are
    _vn.Folded's."""
    NAME, ENTRY = "fold_vn_point", "svnet_vn_point_fold_f32"
    wide = False

    def __init__(self, layer, cloud_channels=0, wide=False):
        self.wide = bool(wide)                           # the envelope the layer was folded in: vn_point launches in the same
        self.ENTRY = _entry("point", "fold_f32", self.wide)
        wf, wd, _ = _vn.check_layer(self.NAME, layer, even=False)
        Cg = int(cloud_channels)
        if Cg < 0 or Cg >= wf.shape[1]:
            raise ValueError("fold_vn_point: cloud_channels = %d of %d input channels: needs 0 <= cloud_channels < the input width" % (Cg, wf.shape[1]))
        self.place(layer)
        self.dims = self.C, self.Cg, self.O, self.Od = int(wf.shape[1]) - Cg, Cg, int(wf.shape[0]), int(wd.shape[0])
        if not supported_point(1, self.C, self.Cg, self.O, self.Od, self.wide):
            max_c, max_o = _widest(self.wide)
            raise _lib.SvnetHipError("fold_vn_point: C = %d, Cg = %d, O = %d is not supported (1 <= C <= %d, Cg <= %d, 1 <= O <= %d)"
                                     % (self.C, self.Cg, self.O, max_c, max_c, max_o))
        self.allocate((self.C + self.Cg) * (self.O + self.Od) + 2 * self.O)

    def cloud_terms(self, B):
        """The workspace of the cloud term for B clouds (uint8; one byte when Cg = 0)."""
        return self._ws.take(int(getattr(_lib.lib(), _entry("point", "workspace_bytes", self.wide))(B, self.Cg, self.O, self.Od)))


def fold_vn_point(layer, cloud_channels=0, wide=False):
    """A VNLinearLeakyReLU on a HIP device whose last `cloud_channels` input channels are constant over a cloud -> FoldedVNPoint.
    wide: fold it in the wide envelope (module docstring, limits); the folded layer carries it."""
    return FoldedVNPoint(layer, cloud_channels, wide)


def _cloud_shape(name, cloud, B, Cg):
    if Cg == 0 and cloud is None:
        return
    if cloud is None or cloud.dim() != 3 or tuple(cloud.shape) != (B, Cg, 3) or Cg == 0:
        raise ValueError("%s: cloud must be [B,Cg,3] = %s%s, got %s" % (name, (B, Cg, 3), " (None with no constant channels)" if Cg == 0 else "",
                                                                        None if cloud is None else tuple(cloud.shape)))


def _launch_point(x, cloud, folded, out, B, N):
    ws = folded.cloud_terms(B)
    with torch.cuda.device(x.device):
        _lib.call(_entry("point", "f32", folded.wide), _call.p(x), _call.p(cloud), _call.p(folded.folded), B, N, folded.C, folded.Cg, folded.O, folded.Od, folded.slope,
                  _call.p(ws), ws.numel() if folded.Cg else 0, _call.p(out), _call.stream())


def vn_point(x, folded, cloud=None, out=None):
    """x [B,C,3,N] float32, folded a FoldedVNPoint over C + Cg -> O, cloud [B,Cg,3] (the channels that are constant over a cloud; None
    with Cg = 0) -> out [B,O,3,N]: the layer's eval-mode forward on [x | cloud expanded over the points] (module docstring).  One
    launch on the current stream, and a small one in front of it with Cg > 0; no host read.  No argument may require grad."""
    name = "vn_point"
    B, C, N, _ = _vn.check_entry(name, _WHAT, {"x": x, "cloud": cloud, "out": out}, ("x", "cloud", "out"), folded, FoldedVNPoint, "vn_tail.fold_vn_point",
                                  per=" per point")
    _cloud_shape(name, cloud, B, folded.Cg)
    shape = (B, folded.O, 3, N)
    _vn.check_out(name, out, shape, "[B,O,3,N]", (x, cloud, out), folded)
    if B > MAX_B or not supported_point(N, C, folded.Cg, folded.O, folded.Od, folded.wide):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, C = %d, O = %d is not supported (B <= %d, 1 <= N <= %d, C <= %d, O <= %d)"
                                 % ((name, B, N, C, folded.O, MAX_B, _pointset.MAX_N) + _widest(folded.wide)))
    if out is None:
        out = torch.empty(*shape, dtype=_F32, device=x.device)
    _launch_point(x, cloud, folded, out, B, N)
    return out


def supported_point_norm(N, C, O, wide=False):
    """Whether the norm-only point kernel takes this layer (module docstring, limits)."""
    return _ask("point_norm", wide, N, C, O)


def supported_point_norm_wide(N, C, O):
    """supported_point_norm in the wide envelope."""
    return supported_point_norm(N, C, O, wide=True)


class FoldedVNPointNorm(_vn.Folded):
    """The folded form of a VNLinear over C -> O vector channels followed by a VNBatchNorm, with no leaky rule: WT [C, O] | s [O] | t [O]
    in one buffer on the layer's device, allocated once.  refresh() and release() as _vn.Folded's; there is no workspace."""
    NAME, ENTRY = "fold_vn_linear_norm", "svnet_vn_point_norm_fold_f32"
    wide = False

    def __init__(self, linear, batchnorm, wide=False):
        from .models.vn_layers import VNBatchNorm, VNLinear
        self.wide = bool(wide)
        self.ENTRY = _entry("point_norm", "fold_f32", self.wide)
        if not isinstance(linear, VNLinear) or not isinstance(batchnorm, VNBatchNorm):
            raise TypeError("%s: needs a VNLinear and a VNBatchNorm, got %s and %s" % (self.NAME, type(linear).__name__, type(batchnorm).__name__))
        w, bn = linear.map_to_feat.weight, batchnorm.bn
        if int(bn.num_features) != w.shape[0]:
            raise ValueError("%s: map_to_feat %s, BatchNorm over %d: the widths differ" % (self.NAME, tuple(w.shape), bn.num_features))
        _vn.check_batchnorm(self.NAME, bn, {"map_to_feat.weight": w})
        self.place(linear)
        self.batchnorm = batchnorm
        self.dims = self.C, self.O = int(w.shape[1]), int(w.shape[0])
        if not supported_point_norm(1, self.C, self.O, self.wide):
            raise _lib.SvnetHipError("%s: C = %d, O = %d is not supported (1 <= C <= %d, 1 <= O <= %d)" % ((self.NAME, self.C, self.O) + _widest(self.wide)))
        self.allocate(self.C * self.O + 2 * self.O)

    def sources(self):
        return [self.layer.map_to_feat.weight], self.batchnorm.bn


def fold_vn_linear_norm(linear, batchnorm, wide=False):
    """A VNLinear and the VNBatchNorm that follows it, on a HIP device -> FoldedVNPointNorm.  wide: as fold_vn_point's."""
    return FoldedVNPointNorm(linear, batchnorm, wide)


def vn_point_norm(x, folded, out=None):
    """x [B,C,3,N] float32, folded a FoldedVNPointNorm over C -> O -> out [B,O,3,N]: the eval-mode forward of the VNBatchNorm on the
    VNLinear's output (module docstring, norm only).  One launch on the current stream, no host read.  No argument may require grad."""
    name = "vn_point_norm"
    B, C, N, _ = _vn.check_entry(name, _WHAT, {"x": x, "out": out}, ("x", "out"), folded, FoldedVNPointNorm, "vn_tail.fold_vn_linear_norm",
                                  per=" per point")
    shape = (B, folded.O, 3, N)
    _vn.check_out(name, out, shape, "[B,O,3,N]", (x, out), folded)
    if B > MAX_B or not supported_point_norm(N, C, folded.O, folded.wide):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, C = %d, O = %d is not supported (B <= %d, 1 <= N <= %d, C <= %d, O <= %d)"
                                 % ((name, B, N, C, folded.O, MAX_B, _pointset.MAX_N) + _widest(folded.wide)))
    if out is None:
        out = torch.empty(*shape, dtype=_F32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call(_entry("point_norm", "f32", folded.wide), _call.p(x), _call.p(folded.folded), B, N, C, folded.O, _call.p(out), _call.stream())
    return out


def vn_cloud_mean(x, out=None, wide=False):
    """x [B,C,3,N] float32 -> out [B,C,3]: the mean over the points in the contract's order (module docstring).  One launch on the
    current stream, no host read.  wide: admit C to MAX_C_WIDE.  No argument may require grad."""
    name = "vn_cloud_mean"
    B, C, N, _ = _vn.check_entry(name, _WHAT, {"x": x, "out": out}, ("x", "out"))
    _vn.check_out(name, out, (B, C, 3), "[B,C,3]", (x, out))
    if B > MAX_B or not supported_point(N, C, 0, 1, 1, wide):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, C = %d is not supported (B <= %d, 1 <= N <= %d, 1 <= C <= %d)"
                                 % (name, B, N, C, MAX_B, _pointset.MAX_N, _widest(wide)[0]))
    if out is None:
        out = torch.empty(B, C, 3, dtype=_F32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call(_entry("cloud_mean", "f32", wide), _call.p(x), B, C, N, _call.p(out), _call.stream())
    return out


_std_workspaces = {}     # device -> _Workspace of vn_std_pool calls that bring none


def vn_std_pool(x, y, w_lin, cloud=None, out=None, workspace=None, wide=False):
    """x [B,C,3,N], y [B,Cy,3,N] (vn2's output), w_lin [3,Cy] (vn_lin.weight as it lies), cloud [B,Cg,3] or None -> out [B, 6 I],
    I = C + Cg: the coordinates of [x | cloud expanded] in the frame w_lin y, pooled [amax | mean] over the points (module docstring).
    Two launches on the current stream, no host read.  workspace: a _Workspace to take the per-run partials from (FusedVNTail's);
    without one the calls of a device share a buffer that grows.  wide: admit C, Cg and Cy to MAX_C_WIDE.  No argument may require
    grad."""
    name = "vn_std_pool"
    B, C, N, _ = _vn.check_entry(name, _WHAT, {"x": x, "y": y, "w_lin": w_lin, "cloud": cloud, "out": out}, ("x", "y", "w_lin", "cloud", "out"))
    Cy = _vn.frame_shapes(name, y, w_lin, B, N)
    Cg = 0 if cloud is None else int(cloud.shape[1]) if cloud.dim() == 3 else -1
    if cloud is not None and (Cg < 1 or tuple(cloud.shape) != (B, Cg, 3)):
        raise ValueError("%s: cloud must be [B,Cg,3] with B = %d, got %s" % (name, B, tuple(cloud.shape)))
    shape = (B, 6 * (C + Cg))
    _vn.check_out(name, out, shape, "[B, 6 (C + Cg)]", (x, y, w_lin, cloud, out))
    if B > MAX_B or not supported_std(N, C, Cg, Cy, wide):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, C = %d, Cg = %d, Cy = %d is not supported (B <= %d, 1 <= N <= %d, C, Cg, Cy <= %d)"
                                 % (name, B, N, C, Cg, Cy, MAX_B, _pointset.MAX_N, _widest(wide)[0]))
    if out is None:
        out = torch.empty(*shape, dtype=_F32, device=x.device)
    if workspace is None:
        workspace = _std_workspaces.setdefault(x.device, _Workspace(x.device))
    ws = workspace.take(int(getattr(_lib.lib(), _entry("std_pool", "workspace_bytes", wide))(B, N, C, Cg)))
    with torch.cuda.device(x.device):
        _lib.call(_entry("std_pool", "f32", wide), _call.p(x), _call.p(cloud), _call.p(y), _call.p(w_lin), B, N, C, Cg, Cy, _call.p(ws), ws.numel(), _call.p(out),
                  _call.stream())
    return out


def supported_coords(N, C, Cy, wide=False):
    """Whether the per-point coordinates kernel takes these widths (vn_std_coords, limits)."""
    return _ask("std_coords", wide, N, C, Cy)


def supported_coords_wide(N, C, Cy):
    """supported_coords in the wide envelope."""
    return supported_coords(N, C, Cy, wide=True)


def vn_std_coords(x, y, w_lin, out=None, wide=False):
    """x [B,C,3,N], y [B,Cy,3,N] (vn2's output), w_lin [3,Cy] (vn_lin.weight as it lies) -> out [B,3C,N]: out[b, 3 i + k, n] is the
    coordinate e[i,k](n) of x[b,i,:,n] in the frame w_lin y, by the frame rows and coordinates rules of the std-pool stage (module
    docstring) - the same device functions, so out.amax(-1) is vn_std_pool's h[:, :3C] bit for bit.  What VN_DGCNN_PSEG's head reads of
    the levels' features.  One launch on the current stream, stores along n, no host read.  1 <= N <= 32768, 1 <= C, Cy <= 512,
    B <= 65535 (`supported_coords`); wide: C, Cy to MAX_C_WIDE.  No argument may require grad."""
    name = "vn_std_coords"
    B, C, N, _ = _vn.check_entry(name, _WHAT, {"x": x, "y": y, "w_lin": w_lin, "out": out}, ("x", "y", "w_lin", "out"))
    Cy = _vn.frame_shapes(name, y, w_lin, B, N)
    shape = (B, 3 * C, N)
    _vn.check_out(name, out, shape, "[B,3C,N]", (x, y, w_lin, out))
    if B > MAX_B or not supported_coords(N, C, Cy, wide):
        raise _lib.SvnetHipError("%s: B = %d, N = %d, C = %d, Cy = %d is not supported (B <= %d, 1 <= N <= %d, 1 <= C, Cy <= %d)"
                                 % (name, B, N, C, Cy, MAX_B, _pointset.MAX_N, _widest(wide)[0]))
    if out is None:
        out = torch.empty(*shape, dtype=_F32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call(_entry("std_coords", "f32", wide), _call.p(x), _call.p(y), _call.p(w_lin), B, N, C, Cy, _call.p(out), _call.stream())
    return out


def std_tail(local, vn1, vn2, w_lin, workspace, wide=False):
    """What follows the local features [B,C,3,N] in every vector-neuron model: the cloud mean, vn1 on [local | mean] with the mean as
    its constant channels, vn2, and the standardise-and-pool stage in the frame w_lin y -> (m [B,C,3], y [B,Cy,3,N], h [B, 12 C]).
    Through the public entries, with their checks; workspace: the caller's _Workspace for the stage's partials.  wide: the mean and
    the pool in the wide envelope (vn1 and vn2 carry their own)."""
    m = vn_cloud_mean(local, wide=wide)
    y = vn_point(vn_point(local, vn1, cloud=m), vn2)
    return m, y, vn_std_pool(local, y, w_lin, cloud=m, workspace=workspace, wide=wide)


class FusedVNTail(_vn.EvalOnly):
    """The eval-mode tail of a VN_DGCNN_CLS on a HIP device: forward(feats) maps the four levels' outputs [B,C_i,3,N] to logits, as
    model.tail does.  The steps: torch.cat of the feats (one copy of 3 x 169 N floats per cloud: 2 % of the tail's traffic - the edge
    levels' entry has no channel window to write into one buffer), conv5, the cloud mean, vn1 with cloud = m, vn2, the
    standardise-and-pool stage, then the head through the model's own linear*, bn* and dp* modules.  `pooled(feats)` is everything in
    front of the head: h [B, 4092].  The three layers are folded at construction; refresh() folds them again after the parameters or
    the running statistics changed; release() frees outgrown workspaces.  Train mode is refused.  A model whose std_feature has
    normalize_frame set, or widths or a call outside the kernels' limits (`supported`), goes through model.tail."""

    def __init__(self, model):
        super().__init__(model)
        std = model.std_feature
        wide = int(model.conv5.map_to_feat.weight.shape[0])
        layers = ((model.conv5, 0), (std.vn1, wide), (std.vn2, 0))
        self.widths = [(int(l.map_to_feat.weight.shape[1]) - cg, cg, int(l.map_to_feat.weight.shape[0]), int(l.map_to_dir.weight.shape[0]))
                       for l, cg in layers]
        self.Cy = int(std.vn_lin.weight.shape[1])
        self.fused = bool(not std.normalize_frame and all(c >= 1 and supported_point(1, c, cg, o, od) for c, cg, o, od in self.widths)
                          and supported_std(1, wide, wide, self.Cy))
        self.layers = [fold_vn_point(l, cg) for l, cg in layers] if self.fused else []
        self._std_ws = _Workspace(self.layers[0].device) if self.fused else None

    def _folded(self):
        return self.layers

    def supported(self, B, N):
        """Whether B clouds of N points take the fused path here; else forward runs model.tail."""
        return bool(self.fused and 1 <= B <= MAX_B and all(supported_point(N, c, cg, o, od) for c, cg, o, od in self.widths)
                    and supported_std(N, self.widths[0][2], self.widths[0][2], self.Cy))

    def _feats(self, feats):
        name = "FusedVNTail"
        self.eval_only()
        feats = list(feats)
        if not feats:
            raise ValueError("%s: feats must hold the levels' outputs [B,C_i,3,N]" % name)
        _pointset.check_tensors(name, {"feats[%d]" % i: f for i, f in enumerate(feats)}, [_F32] * len(feats), _WHAT)
        first = feats[0]
        if any(f.dim() != 4 or f.shape[2] != 3 or f.shape[0] != first.shape[0] or f.shape[3] != first.shape[3] or f.shape[0] < 1 for f in feats):
            raise ValueError("%s: feats must be [B,C_i,3,N] with one B and N, got %s" % (name, [tuple(f.shape) for f in feats]))
        _call.hip(*feats)
        return feats

    @torch.no_grad()
    def pooled(self, feats):
        """The tail in front of the head on the kernels: feats -> h [B, 6 x 682]; raises outside `supported`."""
        feats = self._feats(feats)
        B, N = int(feats[0].shape[0]), int(feats[0].shape[3])
        x = feats[0] if len(feats) == 1 else torch.cat(feats, dim=1)
        if not self.supported(B, N) or int(x.shape[1]) != self.widths[0][0]:
            raise _lib.SvnetHipError("FusedVNTail: B = %d, N = %d, %d channels is outside the fused tail (`supported`)" % (B, N, x.shape[1]))
        _vn.check_model_device("FusedVNTail", self.layers[0], "feats", x)
        conv5, vn1, vn2 = self.layers
        return std_tail(vn_point(x, conv5), vn1, vn2, self.model.std_feature.vn_lin.weight.detach(), self._std_ws)[2]

    @torch.no_grad()
    def forward(self, feats):
        feats = self._feats(feats)
        B, N = int(feats[0].shape[0]), int(feats[0].shape[3])
        if not self.supported(B, N) or sum(int(f.shape[1]) for f in feats) != self.widths[0][0]:
            return self.model.tail(feats)
        h = self.pooled(feats)
        model = self.model
        for layer in (1, 2):
            linear, bn, drop = (getattr(model, "%s%d" % (n, layer)) for n in ("linear", "bn", "dp"))
            h = drop(torch.nn.functional.leaky_relu(bn(linear(h)), negative_slope=0.2))
        return model.linear3(h)
