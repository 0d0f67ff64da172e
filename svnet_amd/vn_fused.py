"""Fused vector-neuron edge level for inference: the point tables, the leaky rule and the mean over the neighbours as two launches
(svnet_amd/csrc/vn_edge.hip), and the eval-mode forward of VN_DGCNN_CLS on top of it.

An edge level of the vector-neuron DGCNN is get_graph_feature -> VNLinearLeakyReLU -> mean over k (svnet_amd/models/vn_layers.py,
models/utils/vn_util.py).  In torch operations it works on [B, 2C, 3, N, k] and [B, O, 3, N, k] tensors and writes and re-reads more
than ten of them; the mean then keeps 1/k.  The level is linear in the edge feature in front of its non-linearity,

    W [x_j - x_i | x_i] = W_a x_j + (W_b - W_a) x_i,

so the products are taken once per point (the tables: k times fewer multiply-adds) and the edge pass is a gather of two table rows,
the non-linearity and a running sum that writes 3 O floats per point and nothing else.  Training is out of scope, as in
svnet_amd/sa_fused.py: the modules stay as they are, this is an entry beside them, for pooling = 'mean'.

    folded = fold_vn_layer(layer)                      # a VNLinearLeakyReLU over 2C -> O; buffers allocated once, refresh()
    out = vn_edge_mean(x, idx, folded, out=None)       # x [B,C,3,N] f32, idx [B,N,k] int64 -> [B,O,3,N]
    out = vn_edge2_mean(x, idx, folded1, folded2)      # two layers per edge in front of the mean (VN_DGCNN_PSEG's levels): its docstring
    fused = FusedVNDGCNN(model, tail=False)            # an nn.Module: the eval-mode forward of a VN_DGCNN_CLS; tail=True: the rest of
                                                       # the network through svnet_amd.vn_tail.FusedVNTail as well
    logits = fused(x)                                  # x [B,3,N]; fused.last_idx: the four neighbour lists of this call

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf;
EPS = fl(1e-6), vn_layers.EPS):

    fold        A_f = W_feat[:, :C], D_f = fl(W_feat[:, C:] - W_feat[:, :C]); A_d, D_d likewise from map_to_dir (O rows, or 1 row
                under share_nonlinearity: Od = 1 and every o uses direction row 0).  From BatchNorm's running statistics, as
                fold_level does: invstd = fl(1 / fl(sqrt(fl(var + eps)))), s = fl(gamma invstd), t = fl(beta - fl(mean s)).
    tables      per point n, component a and row o: four c-ascending chains acc = +0; acc = fmaf(x[c,a,n], M[o,c], acc):
                Pn with M = A_f, Pc with D_f, Qn with A_d, Qc with D_d.  K is never split, so no value depends on tiling.
    edge        (n, j), m = idx[n,j] clamped into 0 .. N-1:  p[o,a] = fl(Pn[m,o,a] + Pc[n,o,a]),  d likewise from Qn, Qc.
    norm        q = fl(p0 p0), then fmaf in p1 and p2;  r = fl(fl(sqrt(q)) + EPS);  nb = fmaf(r, s[o], t[o]);  g = fl(nb / r);
                p'[a] = fl(p[a] g).
    leaky       dot and dd are 3-term chains like q, of p' d and d d.  If dot >= 0 then w = p'; otherwise c = fl(dot / fl(dd + EPS))
                and w[a] = fmaf(-c, d[a], p'[a]).  y[a] = fmaf(slope, p'[a], fl(fl(1 - slope) w[a])).  The function is continuous
                across dot = 0: the mask selects between branches that agree there.
    mean        out[o,a,n] = fl((sum over j ascending from +0 of y_j[o,a]) / fl(k)).
    limits      1 <= k <= 64, k <= N <= 32768, 1 <= C <= 128, 1 <= O <= 128, Od is O or 1 (`supported`).  Inputs are assumed finite.

The module divides by the norm and multiplies by BatchNorm's output, p / r * nb, in batched torch operations; the contract's order
differs from it in rounding only.  tests/vn_ref.py restates the contract in numpy; the kernel's results are compared with it as bit
patterns (a -0 counted as +0).  No argument may require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _lib, _pointset, _vn

__all__ = ["fold_vn_layer", "vn_edge_mean", "vn_edge2_mean", "supported", "supported2", "FoldedVNLayer", "FusedVNDGCNN", "MAX_K", "MAX_C", "MAX_O"]

_WHAT = "the fused vector-neuron edge level"   # in the messages of _pointset.check_tensors
MAX_K, MAX_C, MAX_O = 64, 128, 128


def supported(N, k, C, O, Od):
    """Whether the fused kernels take this level (module docstring, limits)."""
    return bool(_lib.lib().svnet_vn_supported(int(N), int(k), int(C), int(O), int(Od)))


class FoldedVNLayer(_vn.Folded):
    """The folded form of one VNLinearLeakyReLU over 2C -> O vector channels: WT [C, 2 (O + Od)] | s [O] | t [O] in one buffer on the
    layer's device, allocated once, and the table workspace, which grows to the largest (B, N) seen and is then reused (`workspace`:
    the current one).  refresh() and release() are _vn.Folded's: a workspace that was outgrown stays allocated, so a caller that
    sweeps growing (B, N) holds one buffer per growth step (134 MB at B 32, N 1024 for the classifier's widest level) until release()."""
    NAME, ENTRY = "fold_vn_layer", "svnet_vn_fold_f32"

    def __init__(self, layer):
        wf, wd, _ = _vn.check_layer(self.NAME, layer, even=True)
        self.place(layer)
        self.dims = self.C, self.O, self.Od = int(wf.shape[1]) // 2, int(wf.shape[0]), int(wd.shape[0])
        if not supported(1, 1, self.C, self.O, self.Od):
            raise _lib.SvnetHipError("fold_vn_layer: C = %d, O = %d is not supported (1 <= C <= %d, 1 <= O <= %d)" % (self.C, self.O, MAX_C, MAX_O))
        self.allocate(self.C * 2 * (self.O + self.Od) + 2 * self.O)

    def tables(self, B, N):
        """The workspace for B clouds of N points (uint8): the one kept if it is large enough, else a new one that replaces it."""
        return self._ws.take(int(_lib.lib().svnet_vn_workspace_bytes(B, N, self.O, self.Od)))


def fold_vn_layer(layer):
    """A VNLinearLeakyReLU over 2C -> O vector channels (an edge level's), on a HIP device -> FoldedVNLayer."""
    return FoldedVNLayer(layer)


def _launch(x, idx, folded, out, B, N, k, edge=True, tables=True):
    ws = folded.tables(B, N)
    with torch.cuda.device(x.device):
        if tables:
            _lib.call("svnet_vn_tables_f32", _call.p(x), _call.p(folded.folded), B, N, folded.C, folded.O, folded.Od, _call.p(ws), ws.numel(),
                      _call.stream())
        if edge:
            _lib.call("svnet_vn_edge_mean_f32", _call.p(ws), ws.numel(), _call.p(idx), _call.p(folded.folded), B, N, k, folded.C, folded.O,
                      folded.Od, folded.slope, _call.p(out), _call.stream())


def vn_edge_mean(x, idx, folded, out=None):
    """x [B,C,3,N] float32, idx [B,N,k] int64 and folded a FoldedVNLayer over 2C -> O -> out [B,O,3,N]: the mean over the k edges of
    the layer's eval-mode forward on [x_j - x_i | x_i] (module docstring).  Two launches on the current stream, no host read.  Entries
    of idx outside 0 .. N-1 are clamped into the cloud.  No argument may require grad."""
    name = "vn_edge_mean"
    B, C, N, k = _vn.check_entry(name, _WHAT, {"x": x, "idx": idx, "out": out}, ("out",), folded, FoldedVNLayer, "vn_fused.fold_vn_layer")
    shape = (B, folded.O, 3, N)
    _vn.check_out(name, out, shape, "[B,O,3,N]", (x, idx, out), folded)
    if not supported(N, k, C, folded.O, folded.Od):
        raise _lib.SvnetHipError("%s: N = %d, k = %d, C = %d, O = %d is not supported (1 <= k <= %d, k <= N <= %d, C <= %d, O <= %d)"
                                 % (name, N, k, C, folded.O, MAX_K, _pointset.MAX_N, MAX_C, MAX_O))
    if out is None:
        out = torch.empty(*shape, dtype=torch.float32, device=x.device)
    _launch(x, idx, folded, out, B, N, k)
    return out


def supported2(N, k, C, O1, Od1, O2, Od2):
    """Whether the two-layer kernel takes this level (vn_edge2_mean, limits)."""
    return bool(_lib.lib().svnet_vn_edge2_supported(int(N), int(k), int(C), int(O1), int(Od1), int(O2), int(Od2)))


def _launch2(x, idx, folded1, folded2, out, B, N, k):
    ws = folded1.tables(B, N)
    with torch.cuda.device(x.device):
        _lib.call("svnet_vn_tables_f32", _call.p(x), _call.p(folded1.folded), B, N, folded1.C, folded1.O, folded1.Od, _call.p(ws), ws.numel(),
                  _call.stream())
        _lib.call("svnet_vn_edge2_mean_f32", _call.p(ws), ws.numel(), _call.p(idx), _call.p(folded1.folded), _call.p(folded2.folded), B, N, k,
                  folded1.C, folded1.O, folded1.Od, folded2.O, folded2.Od, folded1.slope, folded2.slope, _call.p(out), _call.stream())


def vn_edge2_mean(x, idx, folded1, folded2, out=None):
    """x [B,C,3,N] float32, idx [B,N,k] int64, folded1 a FoldedVNLayer over 2C -> O1 and folded2 a vn_tail.FoldedVNPoint over O1 -> O2
    without constant channels -> out [B,O2,3,N]: the mean over the k edges of the two layers' eval-mode forward on [x_j - x_i | x_i]
    (svnet_amd/csrc/vn_edge2.hip), one edge level of VN_DGCNN_PSEG.  The contract, in the words of the module docstring:

        layer 1   per edge (n, j), m = idx[n,j] clamped: y1[c,a], c < O1 - exactly vn_edge_mean's per-edge y (edge, norm, leaky on
                  folded1 with its slope), before its sum.
        layer 2   per row r of W2 = [W_feat2 | W_dir2] stacked and component a: acc = +0; for c ascending over O1:
                  acc = fmaf(y1[c,a], W2[r,c], acc).  K is never split.  p[o,a] are the feat rows, d[od,a] the dir rows (od = o, or 0
                  with Od2 = 1); y2 = norm, leaky on p, d, s2[o], t2[o] with folded2's slope.
        mean      out[o,a,n] = fl((sum over j ascending from +0 of y2_j[o,a]) / fl(k)).
        limits    1 <= k <= 64, k <= N <= 32768, 1 <= C, O1, O2 <= 128, Od1 is O1 or 1, Od2 is O2 or 1 (`supported2`).

    Two launches on the current stream - the tables of layer 1, then the edge pass, which writes 3 O2 floats per point and nothing
    else: layer 1's outputs stay on the chip - and no host read.  Entries of idx outside 0 .. N-1 are clamped into the cloud.  No
    argument may require grad.  tests/vn_pseg_ref.py restates the contract; results are compared with it as bit patterns."""
    from .vn_tail import FoldedVNPoint
    name = "vn_edge2_mean"
    _vn.check_is(name, "folded1", folded1, FoldedVNLayer, "vn_fused.fold_vn_layer")
    _vn.check_is(name, "folded2", folded2, FoldedVNPoint, "vn_tail.fold_vn_point")
    B, C, N, k = _vn.check_entry(name, _WHAT, {"x": x, "idx": idx, "out": out}, folded=folded1, layer="the first layer")
    if folded2.Cg != 0 or folded2.C != folded1.O:
        raise ValueError("%s: the second layer must take the first one's %d channels and no constant ones, it takes %d + %d"
                         % (name, folded1.O, folded2.C, folded2.Cg))
    shape = (B, folded2.O, 3, N)
    _vn.check_out(name, out, shape, "[B,O2,3,N]", (x, idx, out))
    if folded1.device != x.device or folded2.device != x.device:
        raise ValueError("%s: the layers are on %s and %s, x on %s" % (name, folded1.device, folded2.device, x.device))
    if not supported2(N, k, C, folded1.O, folded1.Od, folded2.O, folded2.Od):
        raise _lib.SvnetHipError("%s: N = %d, k = %d, C = %d, O1 = %d, O2 = %d is not supported (1 <= k <= %d, k <= N <= %d, C <= %d, O1, O2 <= %d)"
                                 % (name, N, k, C, folded1.O, folded2.O, MAX_K, _pointset.MAX_N, MAX_C, MAX_O))
    if out is None:
        out = torch.empty(*shape, dtype=torch.float32, device=x.device)
    _launch2(x, idx, folded1, folded2, out, B, N, k)
    return out


class FusedVNDGCNN(_vn.EvalOnly):
    """The eval-mode forward of a VN_DGCNN_CLS on a HIP device with the module's signature, forward(x [B,3,N], idx=None) -> logits:
    the four edge levels run as knn then vn_edge_mean (or on the four given lists), the rest of the network - conv5, VNStdFeature, the
    pools, the head - through the model's own layers, under no_grad.  It holds the model, so ForwardStep and Distiller take it as
    they take the model.  The levels are folded at construction; refresh() folds them again after the parameters or the running
    statistics changed.  Train mode is refused, and the `training` flag is the model's (_vn.EvalOnly).  A model with pooling = 'max',
    or a call with a level outside the kernels' limits (`supported`), goes through the model's own forward.  `last_idx`: the four
    neighbour lists of the last fused call, so that a comparison can replay them into the model.  release() frees the levels'
    outgrown table workspaces (FoldedVNLayer).
    tail=True: what follows the levels runs through svnet_amd.vn_tail.FusedVNTail (conv5, the cloud mean, VNStdFeature and the pools
    on kernels, the head through the model's layers) instead of model.tail; refresh() and release() reach it."""

    def __init__(self, model, tail=False):
        from .models.vn_layers import mean_pool
        super().__init__(model)
        self.mean = all(pool is mean_pool for _, pool in model.edge_levels())
        self.levels = [fold_vn_layer(conv) for conv, _ in model.edge_levels()] if self.mean else []
        self.last_idx = None
        self.__dict__["tail"] = None                        # (kept out of the module registry: it holds the same model)
        if tail and self.mean:
            from .vn_tail import FusedVNTail
            self.__dict__["tail"] = FusedVNTail(model)

    def _folded(self):
        return self.levels + ([] if self.tail is None else [self.tail])

    def supported(self, N, k):
        """Whether clouds of N points with k neighbours take the fused path here; else forward runs the model."""
        return bool(self.mean and all(supported(N, k, f.C, f.O, f.Od) for f in self.levels))

    @torch.no_grad()
    def forward(self, x, idx=None):
        name = self._begin(_WHAT, x)
        B, N, ks = self._lists(name, x, idx, 4)
        if not all(self.supported(N, k) for k in ks):
            return self.model(x, idx=idx)
        _vn.check_model_device(name, self.levels[0], "x", x)
        feats = self._edge_levels(x, idx, ks, [(level, level.O) for level in self.levels], _launch)
        return self.model.tail(feats) if self.tail is None else self.tail(feats)
