"""Epoch metrics accumulated on the device (svnet_amd/csrc/metrics.hip).

The reference ends every epoch with mean loss, accuracy, class-balanced accuracy and - part segmentation - the mean shape IoU of the
train pass and of the test pass (main_cls_dgcnn.py:187-251, main_partseg_dgcnn.py:185-279, utils.py:68-91): it copies every batch's
predictions to the host and hands the concatenation to sklearn / numpy.  Here one launch per batch adds the batch to a small state
on the device - an int64 confusion matrix (true x predicted), the row count, the float64 loss sum, one float64 shape IoU per cloud -
and the host reads that state ONCE per epoch:

    m = EpochMetrics(40, device)                                        # classification
    m = EpochMetrics(50, device, parts=SHAPENET_PARTS, capacity=len(pool))  # part segmentation: rows = points, shape IoU per cloud
    m.reset()
    train_epoch(step, loader, optimizer, metrics=m)                     # step = TrainStep(..., keep_output=True)
    print(m.result())                                                   # {'loss', 'acc', 'balanced_acc', 'rows', 'invalid', ...}

`finalize` and `merge` are pure host functions of the state (numpy): a multi-rank caller gathers the ranks' states and merges them.
There is no CPU fallback: `update` on anything but HIP tensors raises.
"""
import numpy as np
import torch

from . import _call, _lib

# ShapeNetPart: first part id and number of parts of its 16 categories (the 50 part ids are numbered category by category)
SHAPENET_PARTS = ((0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47),
                  (4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3))

CAT_EMPTY, CAT_INVALID = _lib.DEFINES["SVNET_METRICS_CAT_EMPTY"], _lib.DEFINES["SVNET_METRICS_CAT_INVALID"]
SMOOTHING_EPS = 0.2                    # utils.py:39


class EpochMetrics:
    """num_class: columns of the logits (classes, or parts).  parts=(part_start, part_num) switches to the part-segmentation form
    (logits [B,num_class,N], target = the per-point labels [B,N], label = the clouds' categories [B]); capacity = the clouds of a
    pass, one shape-IoU slot each."""

    def __init__(self, num_class, device, smoothing=True, parts=None, capacity=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("svnet_amd: EpochMetrics needs a HIP (cuda) device, got %s — the product path has no CPU fallback" % device)
        self.C, self.device = int(num_class), device
        if self.C < 2:
            raise ValueError("EpochMetrics: num_class %d < 2" % self.C)
        self.eps = SMOOTHING_EPS if smoothing else 0.0
        self.seg = parts is not None
        if self.seg:
            start, num = (np.asarray(p, dtype=np.int64).reshape(-1) for p in parts)
            if start.shape != num.shape or start.size < 1:
                raise ValueError("EpochMetrics: parts must be (part_start, part_num) of one length")
            if capacity is None or int(capacity) < 1:
                raise ValueError("EpochMetrics: the part-segmentation form needs capacity = the number of shapes in a pass")
            self.num_cat = int(start.size)
            self._parts = torch.from_numpy(np.stack([start, num])).to(device)
        self.capacity = int(capacity) if self.seg else 0
        self._words = self.C * self.C + 3
        assert _lib.lib().svnet_metrics_state_bytes(self.C) == 8 * self._words
        # one buffer, so that state() is one copy: [state | shape_iou (float64 bits) | shape_cat]
        self._buf = torch.empty(self._words + 2 * self.capacity, dtype=torch.int64, device=device)
        self._iou = self._buf[self._words:self._words + self.capacity].view(torch.float64)
        self._cat = self._buf[self._words + self.capacity:]
        self._ws = None
        self.reset()

    def reset(self):
        """Empty state, every shape slot unfilled: one launch on the current stream."""
        _lib.call("svnet_metrics_reset", _call.p(self._buf), self.C, _call.p(self._iou) if self.seg else None,
                  _call.p(self._cat) if self.seg else None, self.capacity, _call.stream())

    def _workspace(self, B, N):
        need = _lib.lib().svnet_metrics_workspace_bytes(B, self.C, N)
        if self._ws is None or self._ws.numel() < need:            # (the first update of a shape; none afterwards)
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def update(self, logits, target, count=None, label=None, first=0):
        """Add one batch: one C call on the current stream, no sync, no host read.  count: the valid leading rows (clouds in the
        part-segmentation form), first: the epoch position of slot 0 (where the clouds' shape IoUs go)."""
        _call.hip(logits, target, label)
        if logits.dtype != torch.float32 or target.dtype != torch.int64 or not logits.is_contiguous() or not target.is_contiguous():
            raise TypeError("EpochMetrics.update: logits must be contiguous float32, target contiguous int64")
        if self.seg:
            if logits.dim() != 3 or logits.shape[1] != self.C or tuple(target.shape) != (logits.shape[0], logits.shape[2]):
                raise ValueError("EpochMetrics.update: logits [B,%d,N] and target [B,N] expected, got %s and %s"
                                 % (self.C, tuple(logits.shape), tuple(target.shape)))
            B, N = int(logits.shape[0]), int(logits.shape[2])
            if label is None or label.dtype != torch.int64 or label.numel() != B or not label.is_contiguous():
                raise ValueError("EpochMetrics.update: the part-segmentation form needs label [B] int64")
            ws = self._workspace(B, N)
            _lib.call("svnet_metrics_seg_f32", _call.p(logits), _call.p(target), _call.p(label), B, self.C, N, _call.p(self._parts[0]),
                      _call.p(self._parts[1]), self.num_cat, B if count is None else int(count), int(first), self.eps, _call.p(self._buf),
                      _call.p(self._iou), _call.p(self._cat), self.capacity, _call.p(ws), ws.numel(), _call.stream())
        else:
            if logits.dim() != 2 or logits.shape[1] != self.C or target.numel() != logits.shape[0]:
                raise ValueError("EpochMetrics.update: logits [R,%d] and target [R] expected, got %s and %s"
                                 % (self.C, tuple(logits.shape), tuple(target.shape)))
            R = int(logits.shape[0])
            ws = self._workspace(R, 0)
            _lib.call("svnet_metrics_cls_f32", _call.p(logits), _call.p(target), R, self.C, R if count is None else int(count), self.eps,
                      _call.p(self._buf), _call.p(ws), ws.numel(), _call.stream())

    def state(self):
        """The state as host numpy arrays - the one device-to-host copy (and sync) of an epoch."""
        buf = self._buf.cpu().numpy()
        C, w, cap = self.C, self._words, self.capacity
        st = {"conf": buf[:C * C].reshape(C, C).copy(), "rows": int(buf[C * C]), "invalid": int(buf[C * C + 1]),
              "loss_sum": float(buf[C * C + 2:w].view(np.float64)[0])}
        if self.seg:
            st["shape_iou"] = buf[w:w + cap].view(np.float64).copy()
            st["shape_cat"] = buf[w + cap:].copy()
        return st

    @staticmethod
    def merge(states):
        """Element-wise sum of the integer and float64 parts of several states (ranks, or passes over disjoint parts of an epoch);
        a shape slot is taken from whichever state filled it."""
        states = list(states)
        out = {"conf": sum(np.asarray(s["conf"], dtype=np.int64) for s in states), "rows": sum(int(s["rows"]) for s in states),
               "invalid": sum(int(s["invalid"]) for s in states), "loss_sum": float(sum(np.float64(s["loss_sum"]) for s in states))}
        if "shape_cat" in states[0]:
            iou, cat = np.array(states[0]["shape_iou"], dtype=np.float64), np.array(states[0]["shape_cat"], dtype=np.int64)
            for s in states[1:]:
                filled = np.asarray(s["shape_cat"]) != CAT_EMPTY
                if (filled & (cat != CAT_EMPTY)).any():
                    raise ValueError("EpochMetrics.merge: a shape slot is filled in two states")
                iou[filled], cat[filled] = np.asarray(s["shape_iou"])[filled], np.asarray(s["shape_cat"])[filled]
            out["shape_iou"], out["shape_cat"] = iou, cat
        return out

    @staticmethod
    def finalize(state):
        """loss = loss_sum / rows, acc = trace / rows (sklearn accuracy_score), balanced_acc = mean recall over the classes that occur in
        the targets (sklearn balanced_accuracy_score); part segmentation: shape_iou = np.mean over the filled slots in slot order (the
        reference's np.mean(calculate_shape_IoU(...)); NaN when a filled slot had an invalid label), class_iou = mean over the
        categories that occur of the category's mean shape IoU."""
        conf = np.asarray(state["conf"], dtype=np.int64)
        rows = int(state["rows"])
        nan = float("nan")
        support = conf.sum(axis=1)
        seen = support > 0
        out = {"loss": float(state["loss_sum"]) / rows if rows else nan,
               "acc": float(np.trace(conf)) / rows if rows else nan,
               "balanced_acc": float(np.mean(np.diag(conf)[seen] / support[seen])) if seen.any() else nan,
               "rows": rows, "invalid": int(state["invalid"])}
        if "shape_cat" in state:
            iou, cat = np.asarray(state["shape_iou"], dtype=np.float64), np.asarray(state["shape_cat"], dtype=np.int64)
            filled = cat != CAT_EMPTY
            out["shapes"] = int(filled.sum())
            out["shape_iou"] = float(np.mean(iou[filled])) if filled.any() else nan
            cats = np.unique(cat[cat >= 0])
            out["class_iou"] = float(np.mean([np.mean(iou[cat == c]) for c in cats])) if cats.size else nan
        return out

    def result(self):
        return self.finalize(self.state())
