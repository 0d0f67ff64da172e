"""The eval-mode forward of BiPointNet_CLS (svnet_amd/models/bipointnet.py) on a fused binary chain: the binary baseline that
`sv_pointnet_cls --binary` is quoted against, and the one model here whose every hot layer is ternary signs against ternary signs.

The module's forward runs one layer per launch and writes every layer's fp32 output - at B 32, N 1024 the 1024-wide layer writes 134 MB
per chain, three times per forward - though that tensor is only ever reduced to its maximum over the cloud, or thresholded by the next
sign().  Here a chain - up to four shared layers over the points, an optional bmm(x^T, T) in front, the write or the maximum behind - is
one launch (svnet_amd/csrc/bi_chain.hip) that keeps the signs in LDS and writes what leaves it.  BiLinearLSR.forward also reads
scale.item() on every call, so the module can never be captured; this forward has no host read and can be.  Training is out of scope.

    folded = fold_bi_layer(linear, bn=None)            # a BiLinearLSR and the BatchNorm1d behind it (or none); refresh()
    first = fold_fp_layer(linear, bn)                  # an nn.Linear with a bias and its BatchNorm1d: a chain's first layer only
    out = bi_chain(x, layers, trans=None, pool=None, offset=0.0, clamp=True, out=None)
                                                       # x [B,C0,N] -> [B,O,N], or [B,O] with pool = 'max'
    fused = FusedBiPointNet(model, logits_only=False)  # an nn.Module: folded at construction; refresh(), release(), supported(B, N)
    logits, trans_feat = fused(x)                      # x [B,3,N]

The contract, for one cloud (fl() is rounding to fp32, every operation rounded once, nothing contracted but the stated fmaf; inputs are
assumed finite; sgn(0) = 0, ternary as everywhere in this library):

    binary fold   m = fl(S / (O K)), S the float64 sum of W in the order include/svnet_hip.h states; S[o,k] = sgn(fl(W[o,k] - m));
                  with BatchNorm invstd and s = fl(gamma invstd) as svnet_sa_fold_f32, a = fl(scale s), b = fl(beta - fl(mean s));
                  without: a = scale, b = +0.
    fp fold       svnet_sa_fold_f32 as it stands; the Linear's bias is its b.
    transform     u[n,j] = +0, then for c ascending u[n,j] = fmaf(x[c,n], T[c,j], u[n,j]); without T, u = x bit for bit.
    fp layer      t[o] = bf[o]; for c ascending t[o] = fmaf(u[c], Wf[o,c], t[o]).
    binary layer  d[o] = sum_c sgn(h[c]) S[o,c], an exact integer; t[o] = fmaf((float)d[o], a[o], b[o]); the next layer reads h = t:
                  sign(hardtanh(t)) = sign(t), so no activation is written between layers.
    write         out[b,o,n] = t, clamped into [-1,1] with clamp (the module's hardtanh).
    max           out[b,o] = fl(max over n < N of t_n[o] + offset): order-free, no float atomics, two runs give the same bits.
    limits        1 <= N <= 32768, 1 <= L <= 4, C0 <= 64 with T or an fp first layer (its width <= 512), every binary input width
                  <= 512, the last width <= 2048, B <= 65535 (`supported`).

tests/bi_ref.py restates the contract in numpy; the kernel's results are compared with it as bit patterns (a -0 counted as +0).  The
fully connected layers behind a maximum act on [B,1024]: they run through svnet_binlinear_fwd_f32 with a as its scale and b as its
bias - exact counts and no .item().  No argument may require grad.  There is no CPU fallback: tensors that are not on a HIP device raise.
"""
import torch

from . import _call, _level, _lib, _pointset, _vn

__all__ = ["fold_bi_layer", "fold_fp_layer", "bi_chain", "supported", "rows_tile", "FoldedBi", "FoldedFp", "FusedBiPointNet", "MAX_LAYERS",
           "MAX_B"]

_WHAT = "the fused binary chain"                  # in the messages of _pointset.check_tensors
_F32 = torch.float32
MAX_LAYERS, MAX_B = 4, 65535


def supported(C0, N, widths, first_fp=False, trans=False):
    """Whether the chain kernel takes a chain of these widths on C0 input channels and N points (module docstring, limits)."""
    L, arr = _level.c_widths(widths)
    return bool(_lib.lib().svnet_bi_chain_supported(int(C0), int(N), L, arr, int(bool(first_fp)), int(bool(trans))))


def rows_tile():
    """Points one workgroup takes: a cloud of more takes further tiles, and a maximum a finishing launch."""
    return int(_lib.lib().svnet_bi_chain_rows_tile())


def _check_bn(name, bn, weights):
    if not isinstance(bn, torch.nn.BatchNorm1d):
        raise TypeError("%s: bn must be a BatchNorm1d, got %s" % (name, type(bn).__name__))
    _vn.check_batchnorm(name, bn, weights)
    if int(bn.num_features) != int(next(iter(weights.values())).shape[0]):
        raise ValueError("%s: a BatchNorm over %d behind %d outputs" % (name, bn.num_features, next(iter(weights.values())).shape[0]))


class FoldedBi:
    """The folded form of one BiLinearLSR over K -> O and the BatchNorm1d behind it, or none: `ab`, a [O] | b [O]; `w_i8`, the signs in
    the chain kernel's packed form (None where K > 512 or O > 2048: such a layer is fully connected only); `w_sign` / `w_nz`, the bit planes the
    binary linear entry reads.  Allocated once on the layer's device; refresh() folds again - after the parameters or the running
    statistics changed - in two launches on the current stream with no host read, so it can be captured."""
    NAME = "fold_bi_layer"

    def __init__(self, linear, bn=None):
        from .models.bipointnet_basic import BiLinearLSR
        if not isinstance(linear, BiLinearLSR):
            raise TypeError("%s: needs a BiLinearLSR, got %s" % (self.NAME, type(linear).__name__))
        if not linear.binary_act:
            raise ValueError("%s: the layer has binary_act = False: its input is not binarized" % self.NAME)
        w, scale = linear.weight, linear.scale
        if w.dtype != _F32 or not w.is_contiguous() or scale.dtype != _F32 or scale.device != w.device or scale.dim() != 0:
            raise ValueError("%s: weight must be contiguous float32 and scale a float32 scalar on %s" % (self.NAME, w.device))
        if bn is not None:
            _check_bn(self.NAME, bn, {"weight": w})
        if float(scale.detach()) == 0.0:
            raise ValueError("%s: the layer's scale is still 0 - run one forward of the module, or reset_scale(input), first" % self.NAME)
        self.device = _pointset.hip_device(self.NAME, w.device)
        self.linear, self.bn = linear, bn
        self.O, self.K = int(w.shape[0]), int(w.shape[1])
        packed = int(_lib.lib().svnet_bi_packed_bytes(self.O, self.K))
        if self.O * self.K > 1 << 24:
            raise _lib.SvnetHipError("%s: %d -> %d is not supported (O K <= 2^24)" % (self.NAME, self.K, self.O))
        words = self.O * ((self.K + 63) // 64)
        self.ab = torch.empty(2 * self.O, dtype=_F32, device=self.device)
        self.w_i8 = torch.empty(packed, dtype=torch.int8, device=self.device) if packed else None
        self._s = torch.empty(self.O, self.K, dtype=_F32, device=self.device)
        self.w_sign = torch.empty(words, dtype=torch.int64, device=self.device)
        self.w_nz = torch.empty(words, dtype=torch.int64, device=self.device)
        self.zeros = torch.zeros(self.K, dtype=_F32, device=self.device)          # the binary linear entry's input shift
        self.refresh()

    def refresh(self):
        lin, bn = self.linear, self.bn
        if lin.weight.device != self.device:
            raise ValueError("%s: the layer moved from %s to %s - fold it again" % (self.NAME, self.device, lin.weight.device))
        stats = [None] * 4 if bn is None else [bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var]
        with torch.cuda.device(self.device):
            _lib.call("svnet_bi_fold_f32", _call.p(lin.weight.detach()), _call.p(lin.scale.detach()), *(_call.p(t) for t in stats), self.O, self.K,
                      float(bn.eps) if bn is not None else 0.0, _call.p(self.w_i8), _call.p(self._s), _call.p(self.ab), _call.stream())
            _lib.call("svnet_binweight_prepare_f32", _call.p(self._s), None, self.O, self.K, _call.p(self.w_sign), _call.p(self.w_nz), None, None,
                      _call.stream())
        return self

    def release(self):
        return self

    def linear_rows(self, h, out=None):
        """h [M,K] float32 -> [M,O]: t = fmaf(d, a, b) per row through svnet_binlinear_fwd_f32 (a as its scale, b as its bias)."""
        M = int(h.shape[0])
        if out is None:
            out = torch.empty(M, self.O, dtype=_F32, device=h.device)
        with torch.cuda.device(self.device):
            _lib.call("svnet_binlinear_fwd_f32", _call.p(h), self.K, _call.p(self.zeros), _call.p(self.w_sign), _call.p(self.w_nz), _call.p(self.ab),
                      _call.p(self.ab[self.O:]), M, self.K, self.O, _call.p(out), None, None, None, _call.stream())
        return out


class FoldedFp:
    """The folded form of one nn.Linear with a bias over K -> O and its BatchNorm1d, svnet_sa_fold_f32's: `w` Wf [O,K], `ab` bf [O]."""
    NAME = "fold_fp_layer"

    def __init__(self, linear, bn):
        from .models.bipointnet_basic import BiLinearLSR
        if not isinstance(linear, torch.nn.Linear) or isinstance(linear, BiLinearLSR):
            raise TypeError("%s: needs a full-precision nn.Linear, got %s" % (self.NAME, type(linear).__name__))
        if linear.bias is None:
            raise ValueError("%s: the Linear must have a bias" % self.NAME)
        _check_bn(self.NAME, bn, {"weight": linear.weight, "bias": linear.bias})
        self.device = _pointset.hip_device(self.NAME, linear.weight.device)
        self.linear, self.bn = linear, bn
        self.O, self.K = int(linear.weight.shape[0]), int(linear.weight.shape[1])
        self.w = torch.empty(self.O, self.K, dtype=_F32, device=self.device)
        self.ab = torch.empty(self.O, dtype=_F32, device=self.device)
        self.refresh()

    def refresh(self):
        lin, bn = self.linear, self.bn
        if lin.weight.device != self.device:
            raise ValueError("%s: the layer moved from %s to %s - fold it again" % (self.NAME, self.device, lin.weight.device))
        with torch.cuda.device(self.device):
            _lib.call("svnet_sa_fold_f32", _call.p(lin.weight.detach()), _call.p(lin.bias.detach()), _call.p(bn.weight.detach()),
                      _call.p(bn.bias.detach()), _call.p(bn.running_mean), _call.p(bn.running_var), self.O, self.K, float(bn.eps), _call.p(self.w),
                      _call.p(self.ab), _call.stream())
        return self

    def release(self):
        return self


def fold_bi_layer(linear, bn=None):
    """A BiLinearLSR on a HIP device and the BatchNorm1d behind it, or none -> FoldedBi.  A scale that is still 0 is refused."""
    return FoldedBi(linear, bn)


def fold_fp_layer(linear, bn):
    """An nn.Linear with a bias on a HIP device and its BatchNorm1d -> FoldedFp: the first layer of a chain."""
    return FoldedFp(linear, bn)


def bi_chain(x, layers, trans=None, pool=None, offset=0.0, clamp=True, out=None, workspace=None):
    """x [B,C0,N] float32 through `layers` - FoldedBi, the first possibly a FoldedFp - with trans [B,C0,C0] or None in front ->
    [B,O,N] (clamped into [-1,1] with clamp), or [B,O] with pool = 'max': the maximum over the cloud plus offset (module docstring).
    On the current stream with no host read: capturable.  workspace: a _vn.Workspace for the tiles' partial maxima of clouds of more
    than rows_tile() points; without one it is allocated per call.  No argument may require grad."""
    name = "bi_chain"
    layers = list(layers) if isinstance(layers, (list, tuple)) else layers
    if not isinstance(layers, list) or not 1 <= len(layers) <= MAX_LAYERS:
        raise ValueError("%s: layers must be a list of 1 .. %d folded layers" % (name, MAX_LAYERS))
    for i, f in enumerate(layers):
        if not isinstance(f, FoldedBi) and not (i == 0 and isinstance(f, FoldedFp)):
            raise TypeError("%s: layers[%d] must be a FoldedBi (bi_fused.fold_bi_layer)%s, got %s"
                            % (name, i, " or a FoldedFp (bi_fused.fold_fp_layer)" if i == 0 else "", type(f).__name__))
    if pool not in (None, "max"):
        raise ValueError("%s: pool must be None or 'max', got %r" % (name, pool))
    args = {k: t for k, t in (("x", x), ("trans", trans), ("out", out)) if t is not None or k == "x"}
    _pointset.check_tensors(name, args, [_F32] * len(args), _WHAT)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("%s: x must be [B,C0,N], got %s" % (name, tuple(x.shape)))
    B, C0, N = (int(v) for v in x.shape)
    if trans is not None and tuple(trans.shape) != (B, C0, C0):
        raise ValueError("%s: trans must be [B,C0,C0] = %s, got %s" % (name, (B, C0, C0), tuple(trans.shape)))
    width = C0
    for i, f in enumerate(layers):
        if f.K != width:
            raise ValueError("%s: layers[%d] takes %d channels, %s has %d" % (name, i, f.K, "x" if i == 0 else "the layer before", width))
        if isinstance(f, FoldedBi) and f.w_i8 is None:
            raise _lib.SvnetHipError("%s: layers[%d] is %d wide at its input: a chain's binary layers take at most 512" % (name, i, f.K))
        width = f.O
    shape = (B, width) if pool else (B, width, N)
    _vn.check_out(name, out, shape, "[B,O]" if pool else "[B,O,N]", [t for t in (x, trans, out) if t is not None])
    for i, f in enumerate(layers):
        if f.device != x.device:
            raise ValueError("%s: layers[%d] is on %s, x on %s" % (name, i, f.device, x.device))
    widths = [f.O for f in layers]
    first_fp = isinstance(layers[0], FoldedFp)
    if B > MAX_B or not supported(C0, N, widths, first_fp, trans is not None):
        raise _lib.SvnetHipError("%s: B = %d, C0 = %d, N = %d, widths %s is not supported (B <= %d, 1 <= N <= %d, C0 <= 64 with trans or an fp "
                                 "first layer of at most 512, binary input widths <= 512, the last width <= 2048)"
                                 % (name, B, C0, N, widths, MAX_B, _pointset.MAX_N))
    if out is None:
        out = torch.empty(*shape, dtype=_F32, device=x.device)
    L, c_w = _level.c_widths(widths)
    c_wp = (_lib.c_p * L)(*((f.w if isinstance(f, FoldedFp) else f.w_i8).data_ptr() for f in layers))
    c_ab = (_lib.c_p * L)(*(f.ab.data_ptr() for f in layers))
    need = int(_lib.lib().svnet_bi_chain_workspace_bytes(B, N, width)) if pool else 0
    ws = None
    if need:
        ws = workspace.take(need) if workspace is not None else torch.empty(need, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("svnet_bi_chain_f32", _call.p(x), _call.p(trans), B, C0, N, L, c_w, int(first_fp), c_wp, c_ab, int(bool(pool)), int(bool(clamp)),
                  float(offset), _call.p(ws), need, _call.p(out), _call.stream())
    return out


class FusedBiPointNet(_vn.EvalOnly):
    """The eval-mode forward of a BiPointNet_CLS on a HIP device with the module's signature, forward(x [B,3,N]) -> (logits, trans_feat)
    - or the logits alone with logits_only, so that ForwardStep and evaluate take it - under no_grad.  The steps of the fused path:

        1.    chain A: x through stn.conv1 (fp) .. conv3, the maximum plus offset_map[N] -> [B,1024];
        2.    stn's fc1 .. fc3 through the binary linear entry, plus the identity -> trans [B,3,3];
        3.    chain B: T = trans, the fp conv1 + bn1, written clamped -> h1 [B,64,N];
        4.    chain C: h1 through fstn.conv1 .. conv3, the maximum plus the offset -> [B,1024];
        5.    fstn's fc1 .. fc3, plus the identity -> trans_feat [B,64,64];
        6.    chain D: h1 with T = trans_feat, conv2, conv3, the maximum plus the offset -> [B,1024];
        7.    the head: fc1, fc2 through the binary linear entry, hardtanh and the fp fc3 in torch.

    No step reads the host, so the whole forward can be captured.  The layers are folded at construction; refresh() folds them again
    after the parameters or the running statistics changed; release() frees outgrown workspaces.  Train mode is refused.  The fused
    path is taken when every Linear but feat.stn.conv1, feat.conv1 and the head's fc3 is a BiLinearLSR with binary_act and a non-zero
    scale, those three are full precision (bi_first and bi_last off), pool = 'ema-max', tnet and the feature transform are on, use_bn
    and affine are on, N is in offset_map and the shape is inside `supported`; otherwise forward runs model(x)."""

    @staticmethod
    def model_class():
        from .models.bipointnet import BasicBiPointNet
        return BasicBiPointNet

    @staticmethod
    def _fusable(model):
        from .models.bipointnet_basic import BiLinearLSR
        enc = model.feat
        if not (enc.tnet and enc.feature_transform and enc.use_bn and model.use_bn and hasattr(enc, "stn") and hasattr(enc, "fstn")):
            return False
        if not (enc.pool == enc.stn.pool == enc.fstn.pool == "ema-max"):
            return False
        plain = [enc.stn.conv1.lin, enc.conv1.lin, model.fc3]
        if any(isinstance(m, BiLinearLSR) or m.bias is None for m in plain):
            return False
        binary = [m for m in model.modules() if isinstance(m, torch.nn.Linear) and all(m is not p for p in plain)]
        if not all(isinstance(m, BiLinearLSR) and m.binary_act and float(m.scale.detach()) != 0.0 for m in binary):
            return False
        norms = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
        return all(m.weight is not None and m.bias is not None and m.running_mean is not None for m in norms)

    def __init__(self, model, logits_only=False):
        super().__init__(model)
        self.logits_only = bool(logits_only)
        self.fused = self._fusable(model)
        self.chains, self.fcs, self.eyes, self._std_ws = {}, {}, {}, None
        if self.fused:
            enc, stn, fstn = model.feat, model.feat.stn, model.feat.fstn
            bi, fp = fold_bi_layer, fold_fp_layer
            self.chains = {"A": [fp(stn.conv1.lin, stn.bn1), bi(stn.conv2.lin, stn.bn2), bi(stn.conv3.lin, stn.bn3)],
                           "B": [fp(enc.conv1.lin, enc.bn1)],
                           "C": [bi(fstn.conv1.lin, fstn.bn1), bi(fstn.conv2.lin, fstn.bn2), bi(fstn.conv3.lin, fstn.bn3)],
                           "D": [bi(enc.conv2.lin, enc.bn2), bi(enc.conv3.lin, enc.bn3)]}
            self.fcs = {"stn": [bi(stn.fc1, stn.bn4), bi(stn.fc2, stn.bn5), bi(stn.fc3)],
                        "fstn": [bi(fstn.fc1, fstn.bn4), bi(fstn.fc2, fstn.bn5), bi(fstn.fc3)],
                        "head": [bi(model.fc1, model.bn1), bi(model.fc2, model.bn2)]}
            device = self.chains["B"][0].device
            self.eyes = {k: torch.eye(k, dtype=_F32, device=device).view(1, k * k) for k in (3, fstn.k)}
            self._std_ws = _vn.Workspace(device)

    def _folded(self):
        return [f for group in list(self.chains.values()) + list(self.fcs.values()) for f in group]

    def supported(self, B, N):
        """Whether B clouds of N points take the fused path here; else forward runs the model."""
        from .models.bipointnet import offset_map
        if not self.fused or not 1 <= B <= MAX_B or N not in offset_map:
            return False
        C = self.chains
        joined = (C["A"][-1].O == self.fcs["stn"][0].K and self.fcs["stn"][-1].O == 9 and C["B"][0].K == 3
                  and C["B"][0].O == C["C"][0].K == C["D"][0].K == self.model.feat.fstn.k and C["C"][-1].O == self.fcs["fstn"][0].K
                  and C["D"][-1].O == self.fcs["head"][0].K and self.fcs["head"][-1].O == self.model.fc3.in_features)
        return bool(joined and supported(3, N, [f.O for f in C["A"]], True, False) and supported(3, N, [f.O for f in C["B"]], True, True)
                    and supported(C["C"][0].K, N, [f.O for f in C["C"]], False, False)
                    and supported(C["D"][0].K, N, [f.O for f in C["D"]], False, True))

    def _tnet(self, pooled, key, k):
        h = pooled
        for f in self.fcs[key]:
            h = f.linear_rows(h)
        return (h + self.eyes[k]).view(-1, k, k)

    @torch.no_grad()
    def encode(self, x):
        """Steps 1 to 7 on the kernels: x [B,3,N] contiguous -> the stages {name: tensor}, "logits" and "trans_feat" among them; raises
        outside `supported`."""
        from .models.bipointnet import offset_map
        B, _, N = (int(v) for v in x.shape)
        if not self.supported(B, N):
            raise _lib.SvnetHipError("FusedBiPointNet: B = %d, N = %d is outside the fused path (`supported`)" % (B, N))
        C, ws, off, st = self.chains, self._std_ws, offset_map[N], {}
        st["pool_stn"] = bi_chain(x, C["A"], pool="max", offset=off, workspace=ws)
        st["trans"] = self._tnet(st["pool_stn"], "stn", 3)
        st["h1"] = bi_chain(x, C["B"], trans=st["trans"], clamp=True)
        st["pool_fstn"] = bi_chain(st["h1"], C["C"], pool="max", offset=off, workspace=ws)
        st["trans_feat"] = self._tnet(st["pool_fstn"], "fstn", self.model.feat.fstn.k)
        st["pool"] = bi_chain(st["h1"], C["D"], trans=st["trans_feat"], pool="max", offset=off, workspace=ws)
        h = st["pool"]
        for f in self.fcs["head"]:
            h = f.linear_rows(h)
        st["fc2"] = h
        st["logits"] = self.model.fc3(torch.clamp(h, -1.0, 1.0))
        return st

    @torch.no_grad()
    def forward(self, x):
        name = self._begin(_WHAT, x)
        _call.hip(x)
        B, N = int(x.shape[0]), int(x.shape[2])
        if not self.supported(B, N):
            logits, trans_feat = self.model(x)
        else:
            _vn.check_model_device(name, self.chains["B"][0], "x", x)
            st = self.encode(x.contiguous())
            logits, trans_feat = st["logits"], st["trans_feat"]
        return logits if self.logits_only else (logits, trans_feat)
