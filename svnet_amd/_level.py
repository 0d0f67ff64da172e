"""What the front ends of the fused inference levels share: set abstraction (svnet_amd/sa_fused.py), feature propagation
(svnet_amd/fp_fused.py) and the global level (svnet_amd/sa_global.py).  Private: the public names live in those modules, FoldedLevel,
fold_level and MAX_LAYERS in sa_fused.  The device side of the same - the layer engine and the launch pieces - is
svnet_amd/csrc/mlp_tile.h.

Here: the folded layers of a level, and the argument checks in the order every entry applies them - the level's type, the tensors,
the shapes, the level's input columns, the window of `out`, then (by _call.hip) the HIP device, the level's device and, in the
entry itself, the kernel's limits.  Which kernel runs, its launch and its limits stay in the three modules.
"""
import torch

from . import _call, _lib, _pointset

MAX_LAYERS = _lib.DEFINES["SVNET_SA_MAX_LAYERS"]


def c_widths(widths):
    """widths -> (L, the int64 array of them) as the library's *_supported and *_rows_tile queries take them."""
    widths = [int(w) for w in widths]
    return len(widths), (_lib.c_i64 * max(len(widths), 1))(*widths)


class FoldedLevel:
    """The folded layers of one level: Wf_l [C_l, C_(l-1)] and bf_l [C_l] on the layers' device, allocated once.  refresh() runs the
    folds again - after the parameters or the running statistics changed - on the current stream, one launch per layer."""

    def __init__(self, convs, bns):
        convs, bns = list(convs), list(bns)
        if len(convs) != len(bns) or not 1 <= len(convs) <= MAX_LAYERS:
            raise ValueError("fold_level: %d convolutions and %d BatchNorms, needs 1 .. %d pairs" % (len(convs), len(bns), MAX_LAYERS))
        last = None
        for i, (conv, bn) in enumerate(zip(convs, bns)):
            w = conv.weight
            if w.dim() < 2 or any(int(v) != 1 for v in w.shape[2:]) or conv.bias is None:
                raise ValueError("fold_level: layer %d must be a 1x1 convolution with a bias, got a weight of %s" % (i, tuple(w.shape)))
            if bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
                raise ValueError("fold_level: BatchNorm %d must be affine and track running statistics" % i)
            if int(bn.num_features) != int(w.shape[0]) or (last is not None and int(w.shape[1]) != last):
                raise ValueError("fold_level: layer %d is %s, BatchNorm over %d, behind a layer of width %s"
                                 % (i, tuple(w.shape), bn.num_features, last))
            tensors = {"weight": w, "bias": conv.bias, "bn.weight": bn.weight, "bn.bias": bn.bias, "running_mean": bn.running_mean,
                       "running_var": bn.running_var}
            for k, t in tensors.items():
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != w.device:
                    raise ValueError("fold_level: layer %d %s must be contiguous float32 on %s" % (i, k, w.device))
            last = int(w.shape[0])
        self.device = _pointset.hip_device("fold_level", convs[0].weight.device)
        self.convs, self.bns = convs, bns
        self.c_in = int(convs[0].weight.shape[1])
        self.widths = tuple(int(c.weight.shape[0]) for c in convs)
        self.wf = [torch.empty(int(c.weight.shape[0]), int(c.weight.shape[1]), dtype=torch.float32, device=self.device) for c in convs]
        self.bf = [torch.empty(w, dtype=torch.float32, device=self.device) for w in self.widths]
        L = len(convs)
        self._c_widths = (_lib.c_i64 * L)(*self.widths)
        self._c_wf = (_lib.c_p * L)(*(t.data_ptr() for t in self.wf))
        self._c_bf = (_lib.c_p * L)(*(t.data_ptr() for t in self.bf))
        self.refresh()

    def refresh(self):
        with torch.cuda.device(self.device):
            for conv, bn, wf, bf in zip(self.convs, self.bns, self.wf, self.bf):
                if conv.weight.device != self.device:
                    raise ValueError("fold_level: the layers moved from %s to %s - fold them again" % (self.device, conv.weight.device))
                _lib.call("svnet_sa_fold_f32", _call.p(conv.weight.detach()), _call.p(conv.bias.detach()), _call.p(bn.weight.detach()),
                          _call.p(bn.bias.detach()), _call.p(bn.running_mean), _call.p(bn.running_var), wf.shape[0], wf.shape[1],
                          float(bn.eps), _call.p(wf), _call.p(bf), _call.stream())
        return self


def fold_level(convs, bns):
    """The 1x1 convolutions (Conv2d or Conv1d with a bias) and BatchNorms of one level, on a HIP device -> FoldedLevel."""
    return FoldedLevel(convs, bns)


# ---- the checks of the functional entries (group_mlp_max, interp_mlp, global_mlp_max), in the order they apply them
def check_is_level(name, level, maker="sa_fused.fold_level"):
    if not isinstance(level, FoldedLevel):
        raise TypeError("%s: level must be a FoldedLevel (%s), got %s" % (name, maker, type(level).__name__))


def check_args(name, what, always, optional=(), views=False):
    """_pointset.check_tensors on the arguments {name: (tensor, dtype)} that are `always` there and on those of `optional` that are
    not None.  views: on contiguous copies - a wrapper takes views, as its module does, and makes them contiguous itself."""
    args = dict(always, **{k: v for k, v in dict(optional).items() if v[0] is not None})
    tensors = {k: t.contiguous() if views and isinstance(t, torch.Tensor) else t for k, (t, _) in args.items()}
    _pointset.check_tensors(name, tensors, [dt for _, dt in args.values()], what)


def _xyz_shape(name, arg, xyz, n, B=None):
    """xyz [B,3,<n>], B >= 1 or the B of the cloud before -> (B, points per cloud)."""
    if xyz.dim() != 3 or xyz.shape[1] != 3 or (xyz.shape[0] < 1 if B is None else xyz.shape[0] != B):
        raise ValueError("%s: %s must be [B,3,%s]%s, got %s" % (name, arg, n, "" if B is None else " with B = %d" % B, tuple(xyz.shape)))
    return int(xyz.shape[0]), int(xyz.shape[2])


def _points_shape(name, arg, points, d, n, B, N):
    """points [B,<d>,<n>] of the cloud's B and N, or None -> its channels, 0 for None."""
    if points is not None and (points.dim() != 3 or points.shape[0] != B or points.shape[2] != N):
        raise ValueError("%s: %s must be [B,%s,%s] with B = %d, %s = %d, got %s" % (name, arg, d, n, B, n, N, tuple(points.shape)))
    return 0 if points is None else int(points.shape[1])


def cloud_shapes(name, xyz, points):
    """Channel-first, as a module receives them: xyz [B,3,N] and points [B,D,N] or None -> (B, N, D)."""
    B, N = _xyz_shape(name, "xyz", xyz, "N")
    return B, N, _points_shape(name, "points", points, "D", "N", B, N)


def cloud_pair_shapes(name, xyz1, xyz2, points1, points2):
    """The dense cloud xyz1 [B,3,N] with points1 [B,D1,N] or None, the sampled one xyz2 [B,3,S] with points2 [B,D2,S] -> (B, N, S, D1, D2)."""
    B, N = _xyz_shape(name, "xyz1", xyz1, "N")
    _, S = _xyz_shape(name, "xyz2", xyz2, "S", B)
    D2 = _points_shape(name, "points2", points2, "D2", "S", B, S)
    return B, N, S, _points_shape(name, "points1", points1, "D1", "N", B, N), D2


def check_c_in(name, level, c_in, given):
    """given: the caller's wording of the columns its arguments make, "xyz and points give 3 + 2"."""
    if level.c_in != c_in:
        raise ValueError("%s: the level takes %d input columns, %s" % (name, level.c_in, given))


def check_window(name, out, c_off, level, B, last, letter=None):
    """The level's channels c_off .. c_off + C_out - 1 inside out [B,C_total,last], or out None and c_off 0 -> int(c_off).  letter: the
    name of the last axis in the message, where it is not 1."""
    c_off, C = int(c_off), level.widths[-1]
    if out is not None and (out.dim() != 3 or out.shape[0] != B or out.shape[2] != last or c_off < 0 or c_off + C > out.shape[1]):
        raise ValueError("%s: out must be [B,C_total,%s] with B = %d%s and channels %d .. %d inside it, got %s"
                         % (name, letter or last, B, ", %s = %d" % (letter, last) if letter else "", c_off, c_off + C - 1, tuple(out.shape)))
    if out is None and c_off:
        raise ValueError("%s: c_off = %d without out" % (name, c_off))
    return c_off


def check_device(name, level, arg, t):
    if level.device != t.device:
        raise ValueError("%s: the level is on %s, %s on %s" % (name, level.device, arg, t.device))


def result(out, level, B, last, device):
    """The caller's out, or a new [B,C_out,last]: allocated behind every check."""
    return torch.empty(B, level.widths[-1], last, dtype=torch.float32, device=device) if out is None else out


class FusedWrapper:
    """What FusedSetAbstraction, FusedFeaturePropagation and FusedGlobalAbstraction share: `module`, its folded `levels`, refresh()
    and the start of a call."""

    def refresh(self):
        for level in self.levels:
            level.refresh()
        return self

    def _begin(self, what, always, optional=()):
        """The train-mode refusal and the tensors' checks (check_args, on views) -> the wrapper's name for the messages."""
        name = type(self).__name__
        if self.module.training:
            raise RuntimeError("%s: the module is in train mode - this is the eval-mode forward (module.eval())" % name)
        check_args(name, what, always, optional, views=True)
        return name
