#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz: the epoch metrics of the REFERENCE on small seeded inputs, recorded once as data.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_metrics_golden          (from the repo root, CPU)

It walks two tiny "epochs" batch by batch exactly as the reference's loops do (main_cls_dgcnn.py:165-251,
main_partseg_dgcnn.py:160-279): predictions by `max(dim)[1]`, `utils.cal_loss` per batch weighted by the batch size, then sklearn's
accuracy_score / balanced_accuracy_score and `utils.calculate_shape_IoU` on the concatenation.  Stored: the inputs (logits, targets)
and the reference's results; no reference source.  The cases hold what is easy to get wrong:
  cls: a class that never occurs in the targets, exact logit ties (the lowest index wins), a short final batch;
  seg: a part absent from both prediction and truth (part IoU 1), predictions outside the cloud's category, ties, a short final batch.
No test imports sklearn or the reference: tests/test_host_metrics.py reads the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch
from sklearn import metrics as skm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from svnet_amd.metrics import SHAPENET_PARTS        # noqa: E402


def ref_utils():
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location("ref_utils", os.path.join(ref, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cls_case(U):
    rng = np.random.default_rng(2024)
    M, C, B = 19, 10, 8                                       # batches of 8, 8, 3
    target = rng.integers(0, C - 1, M)                        # class 9 never occurs in the targets (it is predicted, though)
    logits = rng.standard_normal((M, C)).astype(np.float32)
    logits[np.arange(M), target] += np.where(rng.random(M) < 0.6, 2.5, 0.0).astype(np.float32)
    logits[0, 9] = 9.0
    logits[3, [2, 6]] = logits[3].max() + 1.0                 # a two-way tie for the maximum
    logits[11, :] = 0.25                                      # every class ties
    logits[17, [8, 1, 4]] = 5.0
    pred, true, losses, loss_acc, count = [], [], [], 0.0, 0
    for s in range(0, M, B):
        x, y = torch.from_numpy(logits[s:s + B]), torch.from_numpy(target[s:s + B])
        loss = U.cal_loss(x, y)
        loss_acc += loss.item() * x.shape[0]
        count += x.shape[0]
        losses.append(loss.item())
        pred.append(x.max(dim=1)[1].numpy())
        true.append(y.numpy())
    true, pred = np.concatenate(true), np.concatenate(pred)
    return {"cls_logits": logits, "cls_target": target, "cls_batch": np.int64(B), "cls_pred": pred,
            "cls_conf": skm.confusion_matrix(true, pred, labels=np.arange(C)).astype(np.int64),
            "cls_acc": np.float64(skm.accuracy_score(true, pred)), "cls_balanced_acc": np.float64(skm.balanced_accuracy_score(true, pred)),
            "cls_batch_loss": np.asarray(losses, dtype=np.float64), "cls_loss": np.float64(loss_acc / count)}


def seg_case(U):
    rng = np.random.default_rng(2025)
    start, num = (np.asarray(p) for p in SHAPENET_PARTS)
    M, P, N, B = 7, 50, 32, 3                                 # batches of 3, 3, 1
    label = np.array([0, 10, 3, 15, 1, 10, 4], dtype=np.int64)
    seg = np.stack([start[c] + rng.integers(0, num[c], N) for c in label]).astype(np.int64)
    logits = rng.standard_normal((M, P, N)).astype(np.float32)
    for m in range(M):
        hit = rng.random(N) < 0.7
        logits[m, seg[m], np.arange(N)] += np.where(hit, 4.0, 0.0).astype(np.float32)
    # cloud 1 (category 10: parts 30..35): part 33 absent from the truth and never predicted
    seg[1][seg[1] == 33] = 31
    logits[1, 33, :] = -20.0
    # cloud 2 (category 3: parts 8..11): some points predicted as parts of other categories
    logits[2, 40, :5] = 12.0
    logits[2, 0, 5:8] = 12.0
    # exact ties: the lowest index wins
    logits[4, [6, 7], 0:4] = 15.0
    logits[0, [2, 49], 9] = 15.0
    pred, true, labs, losses, loss_acc, count = [], [], [], [], 0.0, 0
    for s in range(0, M, B):
        seg_pred = torch.from_numpy(logits[s:s + B]).permute(0, 2, 1).contiguous()
        sg = torch.from_numpy(seg[s:s + B])
        loss = U.cal_loss(seg_pred.view(-1, P), sg.view(-1, 1).squeeze())
        loss_acc += loss.item() * seg_pred.shape[0]
        count += seg_pred.shape[0]
        losses.append(loss.item())
        pred.append(seg_pred.max(dim=2)[1].numpy())
        true.append(sg.numpy())
        labs.append(label[s:s + B].reshape(-1))
    true, pred, labs = np.concatenate(true), np.concatenate(pred), np.concatenate(labs)
    ious = np.asarray(U.calculate_shape_IoU(pred, true, labs), dtype=np.float64)
    assert not ((pred[1] == 33) | (true[1] == 33)).any() and ((pred[2] < 8) | (pred[2] > 11)).any()
    cats = np.unique(labs)
    return {"seg_logits": logits, "seg_seg": seg, "seg_label": label, "seg_batch": np.int64(B), "seg_pred": pred,
            "seg_conf": skm.confusion_matrix(true.reshape(-1), pred.reshape(-1), labels=np.arange(P)).astype(np.int64),
            "seg_acc": np.float64(skm.accuracy_score(true.reshape(-1), pred.reshape(-1))),
            "seg_balanced_acc": np.float64(skm.balanced_accuracy_score(true.reshape(-1), pred.reshape(-1))),
            "seg_shape_ious": ious, "seg_iou": np.float64(np.mean(ious)),
            "seg_class_iou": np.float64(np.mean([np.mean(ious[labs == c]) for c in cats])),
            "seg_batch_loss": np.asarray(losses, dtype=np.float64), "seg_loss": np.float64(loss_acc / count)}


def main():
    U = ref_utils()
    out = {}
    out.update(cls_case(U))
    out.update(seg_case(U))
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for k in ("cls_acc", "cls_balanced_acc", "cls_loss", "seg_acc", "seg_balanced_acc", "seg_iou", "seg_class_iou", "seg_loss"):
        print("  %-18s %.17g" % (k, float(out[k])))


if __name__ == "__main__":
    main()
