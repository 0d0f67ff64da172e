"""What the front ends of the fused vector-neuron kernels share - the edge level (svnet_amd/vn_fused.py), the tail (svnet_amd/vn_tail.py),
the part-segmentation forward (svnet_amd/vn_pseg.py) and the PointNet forward (svnet_amd/vn_pointnet.py): the checks on the layers that
are to be folded, the workspace that grows and retires, the folded layer - its buffer, refresh() and release() - the argument checks of
the functional entries in the order they apply them, and the eval-only wrapper of a vector-neuron model: its refresh() and release(),
the start of its call and the loop over its edge levels.  Private: the public names, what a level's buffer holds, which kernels run,
their launches and their limits stay in those four modules.  The device side of the same is svnet_amd/csrc/vn_math.h.
"""
import torch

from . import _call, _lib, _pointset

_F32, _I64 = torch.float32, torch.int64


def check_batchnorm(name, bn, weights):
    """The BatchNorm half of a fold's checks: bn is affine and tracks its statistics, and `weights` {name: tensor} - the linear maps in
    front of it - and its four tensors are contiguous float32 on the first weight's device."""
    if bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
        raise ValueError("%s: the BatchNorm must be affine and track running statistics" % name)
    device = next(iter(weights.values())).device
    for k, t in dict(weights, **{"bn.weight": bn.weight, "bn.bias": bn.bias, "running_mean": bn.running_mean, "running_var": bn.running_var}).items():
        if t.dtype != _F32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s: %s must be contiguous float32 on %s" % (name, k, device))


def check_layer(name, layer, even):
    """(map_to_feat.weight, map_to_dir.weight, the BatchNorm) of a VNLinearLeakyReLU that can be folded; `name` is the caller's in the
    messages, `even`: the input width is an edge feature's 2C."""
    from .models.vn_layers import VNLinearLeakyReLU
    if not isinstance(layer, VNLinearLeakyReLU):
        raise TypeError("%s: needs a VNLinearLeakyReLU, got %s" % (name, type(layer).__name__))
    bn = layer.batchnorm.bn
    wf, wd = layer.map_to_feat.weight, layer.map_to_dir.weight
    if (even and wf.shape[1] % 2) or wf.shape[1] != wd.shape[1] or wd.shape[0] not in (wf.shape[0], 1) or int(bn.num_features) != wf.shape[0]:
        raise ValueError("%s: map_to_feat %s, map_to_dir %s, BatchNorm over %d: needs %s, O or 1 direction rows"
                         % (name, tuple(wf.shape), tuple(wd.shape), bn.num_features, "an even input width 2C" if even else "one input width"))
    check_batchnorm(name, bn, {"map_to_feat.weight": wf, "map_to_dir.weight": wd})
    return wf, wd, bn


class Workspace:
    """A byte buffer that grows to the largest need seen and is then reused.  One that was outgrown stays allocated, because a graph
    captured with it goes on replaying into it, until release()."""

    def __init__(self, device):
        self.device, self.buffer, self._retired = device, None, []

    def take(self, need):
        if self.buffer is None or self.buffer.numel() < need:
            if self.buffer is not None:
                self._retired.append(self.buffer)
            self.buffer = torch.empty(max(int(need), 1), dtype=torch.uint8, device=self.device)
        return self.buffer

    def release(self):
        self._retired.clear()


class Folded:
    """The folded form of one VNLinearLeakyReLU: `folded`, one float32 buffer on the layer's device that ends in s [O] | t [O], and a
    workspace that grows.  refresh() runs the fold again - after the parameters or the running statistics changed - on the current
    stream, one launch.  release() frees the outgrown workspaces (the current one stays): only when no captured graph that was
    recorded with one of them will be replayed again, for it would write into memory that may by then belong to another tensor.
    A subclass states NAME (in the messages), ENTRY (the fold's entry point) and `dims` (the entry's integers); its constructor runs
    check_layer, place(), its own limits, then allocate().  One that folds something else than a VNLinearLeakyReLU states sources()."""

    def place(self, layer):
        self.device = _pointset.hip_device(self.NAME, layer.map_to_feat.weight.device)
        self.layer = layer
        self._ws = Workspace(self.device)

    def allocate(self, floats):
        self.folded = torch.empty(floats, dtype=_F32, device=self.device)
        return self.refresh()

    @property
    def slope(self):
        return float(self.layer.negative_slope)

    @property
    def workspace(self):
        return self._ws.buffer

    def sources(self):
        """(the weights the fold entry reads, in its order and map_to_feat's first; the BatchNorm behind them)."""
        return [self.layer.map_to_feat.weight, self.layer.map_to_dir.weight], self.layer.batchnorm.bn

    def refresh(self):
        weights, bn = self.sources()
        if weights[0].device != self.device:
            raise ValueError("%s: the layer moved from %s to %s - fold it again" % (self.NAME, self.device, weights[0].device))
        with torch.cuda.device(self.device):
            _lib.call(self.ENTRY, *(_call.p(w.detach()) for w in weights), _call.p(bn.weight.detach()), _call.p(bn.bias.detach()),
                      _call.p(bn.running_mean), _call.p(bn.running_var), *self.dims, float(bn.eps), _call.p(self.folded), _call.stream())
        return self

    def release(self):
        self._ws.release()
        return self


# ---- the checks of the functional entries (vn_edge_mean, vn_edge2_mean, vn_edge_cross_mean, vn_point, vn_point_norm, vn_cloud_mean,
# vn_std_pool, vn_std_coords), in the order they apply them: check_entry - the folded argument's type; the tensors' type, dtype, one
# device, contiguity, gradients; x's shape, idx's, the layer's input width - then the entry's own shapes (frame_shapes, a cloud), then
# check_out - `out`, the HIP device (_call.hip), the layer's device - and in the entry itself the kernel's limits and the allocation.
# `name` is the entry's, so every message reads as its own.  Two calls an entry, not one a check: a call costs the small entries time.
def check_is(name, arg, folded, cls, maker):
    if not isinstance(folded, cls):
        raise TypeError("%s: %s must be a %s (%s), got %s" % (name, arg, cls.__name__, maker, type(folded).__name__))


def check_entry(name, what, args, optional=("out",), folded=None, cls=None, maker=None, layer="the layer", per="", channels=None):
    """args {argument: tensor}, "x" among them and first; those of `optional` are left out where they are None; "idx" is int64, the
    others float32.  folded: the layer whose input width x must have - none for an entry without a layer, and with `channels` the
    entry takes that width alone - and with cls and maker its type is checked first.  layer, per: the caller's wording of the width
    refusal, "the first layer", " per point".  -> (B, C, N, k), k None without an idx."""
    if cls is not None and not isinstance(folded, cls):
        check_is(name, "folded", folded, cls, maker)
    for key in optional:
        if args[key] is None:
            del args[key]
    _pointset.check_tensors(name, args, [_I64 if key == "idx" else _F32 for key in args], what)
    x, k = args.get("x"), None
    if x.dim() != 4 or x.shape[2] != 3 or x.shape[0] < 1 or (channels is not None and x.shape[1] != channels):
        if channels is None:
            raise ValueError("%s: x must be [B,C,3,N], got %s" % (name, tuple(x.shape)))
        raise ValueError("%s: x must be [B,%d,3,N], got %s" % (name, channels, tuple(x.shape)))
    B, C, N = int(x.shape[0]), int(x.shape[1]), int(x.shape[3])
    if "idx" in args:
        idx = args["idx"]
        if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != N:
            raise ValueError("%s: idx must be [B,N,k] with B = %d, N = %d, got %s" % (name, B, N, tuple(idx.shape)))
        k = int(idx.shape[2])
    if folded is not None and channels is None and C != folded.C:
        raise ValueError("%s: %s takes %d vector channels%s, x has %d" % (name, layer, folded.C, per, C))
    return B, C, N, k


def frame_shapes(name, y, w_lin, B, N):
    """y [B,Cy,3,N] of the cloud's B and N - what the frame is made of - and w_lin [3,Cy] -> Cy."""
    if y.dim() != 4 or y.shape[0] != B or y.shape[2] != 3 or y.shape[3] != N or y.shape[1] < 1:
        raise ValueError("%s: y must be [B,Cy,3,N] with B = %d, N = %d, got %s" % (name, B, N, tuple(y.shape)))
    Cy = int(y.shape[1])
    if tuple(w_lin.shape) != (3, Cy):
        raise ValueError("%s: w_lin must be [3,Cy] = %s (normalize_frame = False), got %s" % (name, (3, Cy), tuple(w_lin.shape)))
    return Cy


def check_out(name, out, shape, letters, tensors, folded=None):
    """out is None or of `shape`, which the message spells `letters`; the entry's `tensors` are on a HIP device; a folded layer is on
    theirs.  What follows in the entry: the kernel's limits, then the allocation of a missing out - behind every check."""
    if out is not None and tuple(out.shape) != shape:
        raise ValueError("%s: out must be %s = %s, got %s" % (name, letters, shape, tuple(out.shape)))
    _call.hip(*tensors)
    if folded is not None and folded.device != tensors[0].device:
        raise ValueError("%s: the layer is on %s, x on %s" % (name, folded.device, tensors[0].device))


def check_model_device(name, folded, arg, t):
    """A wrapper's: its model's folded layer against the argument `arg` of a call that takes the fused path."""
    if folded.device != t.device:
        raise ValueError("%s: the model is on %s, %s on %s" % (name, folded.device, arg, t.device))


class EvalOnly(torch.nn.Module):
    """A wrapper that holds a vector-neuron model - a VN_DGCNN_CLS, or what a subclass names in model_class() - and computes its
    eval-mode forward.  Its own `training` flag is the model's at construction
    (a new nn.Module starts in train mode) and follows train() / eval() called on the wrapper; eval_only() reads the model's flag, so
    a mode set on the model directly is honoured as well.  Train mode is refused: batch statistics are not what the kernels compute.
    A subclass lists its folded layers in _folded() and keeps the workspace of its standardise-and-pool stage in `_std_ws`;
    refresh() and release() reach both.  _begin(), _lists() and _edge_levels() are the start of a model wrapper's forward and its
    loop over the edge levels."""

    _std_ws = None

    @staticmethod
    def model_class():
        from .models.vn_dgcnn_cls import VN_DGCNN_CLS
        return VN_DGCNN_CLS

    def __init__(self, model):
        super().__init__()
        cls = self.model_class()
        if not isinstance(model, cls):
            raise TypeError("%s: needs a %s, got %s" % (type(self).__name__, cls.__name__, type(model).__name__))
        self.model = model
        self.training = model.training

    def eval_only(self):
        if self.model.training:
            raise RuntimeError("%s: the model is in train mode - this is the eval-mode forward (model.eval())" % type(self).__name__)

    def _folded(self):
        """What refresh() and release() reach: the folded layers, and a wrapper inside this one."""
        return []

    def refresh(self):
        for f in self._folded():
            f.refresh()
        return self

    def release(self):
        for f in self._folded():
            f.release()
        if self._std_ws is not None:
            self._std_ws.release()
        return self

    def _begin(self, what, x, **more):
        """The start of forward(x [B,3,N], **more): the train-mode refusal, the gradient question - asked of the arguments themselves:
        under no_grad a contiguous copy takes no gradient - the tensors' checks on contiguous copies (a view is taken, as the model
        takes it) and x's shape -> the wrapper's name for the messages."""
        name = type(self).__name__
        self.eval_only()
        args = dict(x=x, **more)
        for key, t in args.items():
            if isinstance(t, torch.Tensor) and t.requires_grad:      # (with one argument the message names it twice, as check_tensors does)
                raise ValueError("%s: %s requires grad - %s is forward only%s" % (name, key, what, "" if more else " in " + key))
        _pointset.check_tensors(name, {key: t.contiguous() if isinstance(t, torch.Tensor) else t for key, t in args.items()}, [_F32] * len(args), what)
        if x.dim() != 3 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError("%s: x must be [B,3,N], got %s" % (name, tuple(x.shape)))
        return name

    @staticmethod
    def is_list(i, B, N):
        """Whether i is a neighbour list of a call on B clouds of N points: an int64 tensor [B,N,k]."""
        return isinstance(i, torch.Tensor) and i.dtype == torch.int64 and i.dim() == 3 and tuple(i.shape[:2]) == (B, N)

    def _lists(self, name, x, idx, levels, others=()):
        """idx: None, or one neighbour list for each of the `levels` edge levels.  Their validation, their device against x's, then
        _call.hip on x, `others` and the lists -> (B, N, the levels' k: the model's without lists)."""
        B, N = int(x.shape[0]), int(x.shape[2])
        lists = () if idx is None else idx
        if idx is not None and (len(idx) != levels or not all(self.is_list(i, B, N) for i in idx)):
            raise ValueError("%s: idx must hold the %s levels' neighbour lists [B,N,k] int64" % (name, {3: "three", 4: "four"}.get(levels, levels)))
        for n, i in enumerate(lists):
            if i.device != x.device:
                raise ValueError("%s: x on %s, idx[%d] on %s" % (name, x.device, n, i.device))
        _call.hip(x, *others, *lists)
        return B, N, [self.model.k] * levels if idx is None else [int(i.shape[2]) for i in idx]

    def _edge_levels(self, x, idx, ks, levels, launch):
        """The edge levels of a DGCNN on x [B,3,N]: per (level, its output width) of `levels` knn on the level's input or the given
        list, a new [B,O,3,N] and launch(h, nbr, level, out, B, N, k).  Sets `last_idx` -> the levels' outputs."""
        from .models.utils.vn_util import knn
        B, _, N = (int(v) for v in x.shape)
        h = x.contiguous().view(B, 1, 3, N)
        feats, used = [], []
        for i, (level, O) in enumerate(levels):
            nbr = knn(h.view(B, -1, N), ks[i]) if idx is None else idx[i].contiguous()
            out = torch.empty(B, O, 3, N, dtype=_F32, device=x.device)
            launch(h, nbr, level, out, B, N, ks[i])
            used.append(nbr)
            feats.append(out)
            h = out
        self.last_idx = used
        return feats
