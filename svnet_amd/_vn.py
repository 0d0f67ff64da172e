"""What the front ends of the fused vector-neuron kernels share, the edge level (svnet_amd/vn_fused.py) and the tail
(svnet_amd/vn_tail.py): the checks on a VNLinearLeakyReLU that is to be folded, the workspace that grows and retires, the folded layer
- its buffer, refresh() and release() - and the eval-only wrapper of a vector-neuron model.  Private: the public names, what a level's buffer
holds, which kernels run and their limits stay in those two modules.  The device side of the same is svnet_amd/csrc/vn_math.h.
"""
import torch

from . import _call, _lib, _pointset

_F32 = torch.float32


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
    if bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
        raise ValueError("%s: the BatchNorm must be affine and track running statistics" % name)
    for k, t in {"map_to_feat.weight": wf, "map_to_dir.weight": wd, "bn.weight": bn.weight, "bn.bias": bn.bias,
                 "running_mean": bn.running_mean, "running_var": bn.running_var}.items():
        if t.dtype != _F32 or not t.is_contiguous() or t.device != wf.device:
            raise ValueError("%s: %s must be contiguous float32 on %s" % (name, k, wf.device))
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
    check_layer, place(), its own limits, then allocate()."""

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

    def refresh(self):
        layer, bn = self.layer, self.layer.batchnorm.bn
        if layer.map_to_feat.weight.device != self.device:
            raise ValueError("%s: the layer moved from %s to %s - fold it again" % (self.NAME, self.device, layer.map_to_feat.weight.device))
        with torch.cuda.device(self.device):
            _lib.call(self.ENTRY, _call.p(layer.map_to_feat.weight.detach()), _call.p(layer.map_to_dir.weight.detach()),
                      _call.p(bn.weight.detach()), _call.p(bn.bias.detach()), _call.p(bn.running_mean), _call.p(bn.running_var), *self.dims,
                      float(bn.eps), _call.p(self.folded), _call.stream())
        return self

    def release(self):
        self._ws.release()
        return self


class EvalOnly(torch.nn.Module):
    """A wrapper that holds a vector-neuron model - a VN_DGCNN_CLS, or what a subclass names in model_class() - and computes its
    eval-mode forward.  Its own `training` flag is the model's at construction
    (a new nn.Module starts in train mode) and follows train() / eval() called on the wrapper; eval_only() reads the model's flag, so
    a mode set on the model directly is honoured as well.  Train mode is refused: batch statistics are not what the kernels compute."""

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
