"""CPU tests of the epoch metrics' host side (svnet_amd/metrics.py): finalize / merge against the reference's recorded results
(tests/golden/metrics.npz, written by tests/golden/make_metrics_golden.py from the reference's loops, sklearn and numpy), the numpy
restatement of the kernels (tests/metrics_ref.py) pinned to the same fixture, and the new entry points' argument errors."""
import ctypes
import os

import numpy as np
import pytest

from tests import metrics_ref as MR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
# acc / balanced_acc: the same integers divided and averaged in another order than sklearn's: float64 rounding only
REL = 1e-15
# the reference's epoch loss is fp32 work (log_softmax over C <= 50 columns, a mean over <= 96 rows, each operation 2^-24 relative, a
# few hundred of them in a chain at worst: < 2e-5) against the restatement's float64
REF_LOSS_REL = 2e-5


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def _rel(a, b):
    return abs(a - b) / abs(b)


def _cls_states(G):
    B = int(G["cls_batch"])
    M = G["cls_logits"].shape[0]
    out = []
    for s in range(0, M, B):
        # fixed [B,C] buffers as a loader fills them: the slots past a short final batch repeat slot 0 and are not counted
        x, y = np.repeat(G["cls_logits"][:1], B, axis=0), np.repeat(G["cls_target"][:1], B)
        n = min(B, M - s)
        x[:n], y[:n] = G["cls_logits"][s:s + n], G["cls_target"][s:s + n]
        out.append(MR.cls_update(MR.new_state(x.shape[1]), x, y, count=n))
    return out


def _seg_states(G):
    from svnet_amd.metrics import SHAPENET_PARTS
    B = int(G["seg_batch"])
    M, P, N = G["seg_logits"].shape
    out = []
    for s in range(0, M, B):
        n = min(B, M - s)
        x, sg, lab = (np.repeat(G[k][:1], B, axis=0) for k in ("seg_logits", "seg_seg", "seg_label"))
        x[:n], sg[:n], lab[:n] = G["seg_logits"][s:s + n], G["seg_seg"][s:s + n], G["seg_label"][s:s + n]
        out.append(MR.seg_update(MR.new_state(P, capacity=M), x, sg, lab, SHAPENET_PARTS, count=n, first=s))
    return out


def test_fixture_holds_the_cases_that_are_easy_to_get_wrong(G):
    from svnet_amd.metrics import SHAPENET_PARTS
    start, num = SHAPENET_PARTS
    assert G["cls_conf"].sum(axis=1)[9] == 0 and G["cls_conf"][:, 9].sum() > 0                 # a class never in the targets, but predicted
    x = G["cls_logits"]
    assert ((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= 3                    # exact ties
    assert x.shape[0] % int(G["cls_batch"]) and G["seg_logits"].shape[0] % int(G["seg_batch"])  # short final batches
    pred, seg, lab = G["seg_pred"], G["seg_seg"], G["seg_label"]
    absent = [(m, p) for m in range(len(lab)) for p in range(start[lab[m]], start[lab[m]] + num[lab[m]])
              if not ((pred[m] == p) | (seg[m] == p)).any()]
    assert (1, 33) in absent                                                                    # a part absent from both: IoU 1
    outside = [(pred[m] < start[lab[m]]) | (pred[m] >= start[lab[m]] + num[lab[m]]) for m in range(len(lab))]
    assert outside[2].any()                                                                     # predictions outside the category
    xs = G["seg_logits"]
    assert ((xs == xs.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()


def test_shapenet_parts_table():
    from svnet_amd.metrics import SHAPENET_PARTS
    start, num = SHAPENET_PARTS
    assert len(start) == len(num) == 16 and sum(num) == 50
    assert list(start) == [sum(num[:i]) for i in range(16)]


def test_finalize_reproduces_the_reference_cls(G):
    from svnet_amd.metrics import EpochMetrics
    st = {"conf": G["cls_conf"], "rows": int(G["cls_conf"].sum()), "invalid": 0, "loss_sum": float(G["cls_loss"]) * int(G["cls_conf"].sum())}
    r = EpochMetrics.finalize(st)
    assert r["rows"] == G["cls_logits"].shape[0] and r["invalid"] == 0
    assert _rel(r["acc"], float(G["cls_acc"])) <= REL and _rel(r["balanced_acc"], float(G["cls_balanced_acc"])) <= REL
    assert _rel(r["loss"], float(G["cls_loss"])) <= REL
    assert "shape_iou" not in r


def test_finalize_reproduces_the_reference_seg(G):
    from svnet_amd.metrics import EpochMetrics
    M = G["seg_logits"].shape[0]
    st = {"conf": G["seg_conf"], "rows": int(G["seg_conf"].sum()), "invalid": 0, "loss_sum": 0.0, "shape_iou": G["seg_shape_ious"],
          "shape_cat": G["seg_label"]}
    r = EpochMetrics.finalize(st)
    assert r["rows"] == G["seg_seg"].size and r["shapes"] == M
    assert _rel(r["acc"], float(G["seg_acc"])) <= REL and _rel(r["balanced_acc"], float(G["seg_balanced_acc"])) <= REL
    assert r["shape_iou"] == float(G["seg_iou"])                       # np.mean of the same values in the same order: the same bits
    assert _rel(r["class_iou"], float(G["seg_class_iou"])) <= REL
    # unfilled slots do not count; an invalid cloud's NaN does
    st2 = dict(st, shape_iou=np.append(G["seg_shape_ious"], [0.0, 0.0]), shape_cat=np.append(G["seg_label"], [-1, -1]))
    assert EpochMetrics.finalize(st2)["shape_iou"] == float(G["seg_iou"]) and EpochMetrics.finalize(st2)["shapes"] == M
    st3 = dict(st, shape_iou=np.append(G["seg_shape_ious"], np.nan), shape_cat=np.append(G["seg_label"], -2))
    assert np.isnan(EpochMetrics.finalize(st3)["shape_iou"]) and not np.isnan(EpochMetrics.finalize(st3)["class_iou"])
    empty = EpochMetrics.finalize({"conf": np.zeros((3, 3), dtype=np.int64), "rows": 0, "invalid": 4, "loss_sum": 0.0})
    assert np.isnan(empty["loss"]) and np.isnan(empty["acc"]) and np.isnan(empty["balanced_acc"]) and empty["invalid"] == 4


def test_restatement_equals_the_reference_cls(G):
    """tests/metrics_ref.py batch by batch (short final batch: count < B), merged: the reference's integers exactly."""
    from svnet_amd.metrics import EpochMetrics
    assert np.array_equal(MR.predict(G["cls_logits"]), G["cls_pred"])
    states = _cls_states(G)
    assert len(states) == 3 and states[-1]["rows"] == 3
    st = EpochMetrics.merge(states)
    assert np.array_equal(st["conf"], G["cls_conf"]) and st["conf"].dtype == np.int64
    assert st["rows"] == G["cls_logits"].shape[0] and st["invalid"] == 0
    r = EpochMetrics.finalize(st)
    assert _rel(r["acc"], float(G["cls_acc"])) <= REL and _rel(r["balanced_acc"], float(G["cls_balanced_acc"])) <= REL
    assert _rel(r["loss"], float(G["cls_loss"])) <= REF_LOSS_REL
    B = int(G["cls_batch"])
    for i, s in enumerate(states):
        assert _rel(s["loss_sum"] / s["rows"], float(G["cls_batch_loss"][i])) <= REF_LOSS_REL, i
    assert B * (len(states) - 1) + states[-1]["rows"] == st["rows"]


def test_restatement_equals_the_reference_seg(G):
    from svnet_amd.metrics import EpochMetrics
    M, P, N = G["seg_logits"].shape
    assert np.array_equal(MR.predict(G["seg_logits"].transpose(0, 2, 1).reshape(-1, P)).reshape(M, N), G["seg_pred"])
    states = _seg_states(G)
    st = EpochMetrics.merge(states)
    assert np.array_equal(st["conf"], G["seg_conf"]) and st["rows"] == M * N and st["invalid"] == 0
    assert np.array_equal(st["shape_iou"].view(np.int64), G["seg_shape_ious"].view(np.int64))          # bit for bit
    assert np.array_equal(st["shape_cat"], G["seg_label"])
    r = EpochMetrics.finalize(st)
    assert r["shape_iou"] == float(G["seg_iou"])
    assert _rel(r["acc"], float(G["seg_acc"])) <= REL and _rel(r["balanced_acc"], float(G["seg_balanced_acc"])) <= REL
    assert _rel(r["loss"], float(G["seg_loss"])) <= REF_LOSS_REL
    # merging the batches as two ranks would hold them (0 and 2 | 1) gives the same state
    two = EpochMetrics.merge([EpochMetrics.merge([states[0], states[2]]), states[1]])
    assert np.array_equal(two["conf"], st["conf"]) and np.array_equal(two["shape_iou"].view(np.int64), st["shape_iou"].view(np.int64))
    assert np.array_equal(two["shape_cat"], st["shape_cat"]) and two["rows"] == st["rows"]
    with pytest.raises(ValueError):
        EpochMetrics.merge([states[0], states[0]])                    # one slot filled twice


def test_restatement_skips_invalid_rows_and_poisons_invalid_clouds(G):
    from svnet_amd.metrics import SHAPENET_PARTS
    x, sg, lab = G["seg_logits"][:3].copy(), G["seg_seg"][:3].copy(), G["seg_label"][:3].copy()
    sg[0, :5], sg[2, 7] = -1, 50
    lab[1] = 16
    st = MR.seg_update(MR.new_state(50, capacity=4), x, sg, lab, SHAPENET_PARTS, first=1)
    assert st["invalid"] == 6 and st["rows"] == 3 * x.shape[2] - 6 and st["conf"].sum() == st["rows"]
    assert np.isnan(st["shape_iou"][2]) and list(st["shape_cat"]) == [-1, lab[0], -2, lab[2]] and np.isfinite(st["shape_iou"][[1, 3]]).all()
    c = MR.cls_update(MR.new_state(10), G["cls_logits"][:4], np.array([1, -1, 10, 3]))
    assert c["invalid"] == 2 and c["rows"] == 2 and c["conf"].sum() == 2
    nan_row = np.array([[0.0, np.nan, 5.0, np.nan]], dtype=np.float32)
    assert MR.predict(nan_row)[0] == 1                                # the first NaN is the maximum


def test_loss_bound_is_small_and_positive(G):
    b = MR.loss_bound(G["cls_logits"], G["cls_target"])
    assert 0 < b < 1e-3 * MR.loss_terms(G["cls_logits"], G["cls_target"]).sum()


def test_argument_errors_of_the_metrics_entries_do_not_need_a_gpu():
    from svnet_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)                    # never dereferenced: every call below is refused on the host
    assert L.svnet_metrics_state_bytes(40) == (40 * 40 + 3) * 8 and L.svnet_metrics_state_bytes(1) == 0
    assert L.svnet_metrics_workspace_bytes(32, 40, 0) >= 8 * 8 and L.svnet_metrics_workspace_bytes(32, 50, 2048) >= 32 * 8 * 8 + 32 * 2 * 50 * 4
    assert L.svnet_metrics_workspace_bytes(0, 40, 0) == 0
    assert L.svnet_metrics_reset(None, 40, None, None, 0, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_metrics_reset(p, 40, None, None, 5, None) == -1
    assert L.svnet_metrics_cls_f32(None, p, 4, 40, 4, 0.2, p, p, 1 << 20, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_metrics_cls_f32(p, p, 4, 1, 4, 0.2, p, p, 1 << 20, None) == -1
    assert L.svnet_metrics_cls_f32(p, p, 4, 40, 5, 0.2, p, p, 1 << 20, None) == -1 and b"count" in L.svnet_last_error()
    assert L.svnet_metrics_cls_f32(p, p, 4, 40, 4, 1.5, p, p, 1 << 20, None) == -1
    assert L.svnet_metrics_cls_f32(p, p, 4, 40, 4, 0.2, p, p, 4, None) == -3 and b"workspace" in L.svnet_last_error()
    assert L.svnet_metrics_cls_f32(p, p, 4, 40, 4, 0.2, p, None, 0, None) == -3

    def seg(logits=p, B=4, P=50, N=128, count=4, first=0, capacity=8, ws=p, ws_bytes=1 << 24, iou=p):
        return L.svnet_metrics_seg_f32(logits, p, p, B, P, N, p, p, 16, count, first, 0.2, p, iou, p, capacity, ws, ws_bytes, None)
    assert seg(logits=None) == -1 and b"null" in L.svnet_last_error()
    assert seg(iou=None) == -1
    assert seg(P=1) == -1 and seg(N=0) == -1 and seg(count=5) == -1 and seg(first=-1) == -1
    assert seg(first=5) == -2 and b"capacity" in L.svnet_last_error()            # first + count > capacity
    assert seg(P=4097) == -2 and seg(B=65536, count=1, capacity=1 << 20) == -2
    assert seg(ws_bytes=16) == -3 and seg(ws=None) == -3
