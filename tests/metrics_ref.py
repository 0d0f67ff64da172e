"""numpy restatement of svnet_amd/csrc/metrics.hip (svnet_metrics_cls_f32 / svnet_metrics_seg_f32): what one update adds to the state,
in integers and float64, written independently of the kernels.  tests/test_host_metrics.py pins it to the reference's recorded results
(tests/golden/metrics.npz); the GPU tests compare the kernels with it at arbitrary shapes.

A state is the dict EpochMetrics.state() returns: conf [C,C] int64 (true x predicted), rows, invalid, loss_sum and, for part
segmentation, shape_iou [capacity] float64 / shape_cat [capacity] int64 (-1 = unfilled, -2 = a cloud with an invalid label)."""
import numpy as np

EPS = float(np.float32(0.2))          # the kernel's eps argument is a float
U = 2.0 ** -23                        # one fp32 ulp relative to the value: at least twice the rounding error of any single fp32 operation


def new_state(C, capacity=None):
    st = {"conf": np.zeros((C, C), dtype=np.int64), "rows": 0, "invalid": 0, "loss_sum": 0.0}
    if capacity is not None:
        st["shape_iou"] = np.full(capacity, np.nan)
        st["shape_cat"] = np.full(capacity, -1, dtype=np.int64)
    return st


def predict(x):
    """x [R,C] -> [R]: the lowest index among the row's maxima, a NaN counting as the maximum (torch.max(dim) on the CPU)."""
    x = np.asarray(x)
    nan = np.isnan(x)
    clean = np.where(nan, -np.inf, x)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), clean.argmax(axis=1)).astype(np.int64)     # (argmax: the first occurrence)


def loss_terms(x, t, eps=EPS):
    """cal_loss's per-row terms -(soft . log_softmax(x)) in float64; x [R,C] float32, t [R] valid targets."""
    x = np.asarray(x, dtype=np.float64)
    R, C = x.shape
    mx = x.max(axis=1, keepdims=True)
    logp = x - (np.log(np.exp(x - mx).sum(axis=1, keepdims=True)) + mx)
    soft = np.full((R, C), eps / (C - 1))
    soft[np.arange(R), t] = 1.0 - eps
    return -(soft * logp).sum(axis=1)


def loss_bound(x, t, eps=EPS):
    """Bound on |fp32 kernel loss_sum - float64 loss_sum| over the rows x [R,C] with valid targets t, from the kernel's arithmetic
    (mx; se = sum expf(x - mx); lse = logf(se) + mx; term = -sum soft_c * (x_c - lse)), each fp32 operation and each of expf / logf
    (1 ulp) counted as a relative error of at most U = 2^-23.  With D = max_c |x_c - mx|, T = the row's term (all addends of one sign,
    so no partial sum exceeds T):
        x_c - mx: U D absolute -> expf of it: relative U D + U;  se: at most C - 1 inexact additions: relative (C - 1) U
        logf(se): absolute (C + D) U + U log C   (se <= C);  + mx: U (|mx| + log C)              => lse off by (C + D + |mx| + 2 log C) U
        x_c - lse: U |logp_c| more; soft weights sum to 1                                         => sum soft_c err(logp_c) <= err(lse) + U T
        on = 1 - eps, off = eps / (C - 1): U each -> U T; products and the C additions of the row sum: (C + 1) U T
    row bound = U (C + D + |mx| + 2 log C + (C + 3) T); the float64 work on top (partials, finishing sum) is below 2^-40 of it."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[1]
    mx = x.max(axis=1)
    D = (mx[:, None] - x).max(axis=1)
    T = loss_terms(x, t, eps)
    return float((U * (C + D + abs(mx) + 2 * np.log(C) + (C + 3) * T)).sum())


def _add_rows(st, x, t, eps):
    C = st["conf"].shape[0]
    ok = (t >= 0) & (t < C)
    st["invalid"] += int((~ok).sum())
    st["rows"] += int(ok.sum())
    if ok.any():
        np.add.at(st["conf"], (t[ok], predict(x[ok])), 1)
        st["loss_sum"] += float(loss_terms(x[ok], t[ok], eps).sum())


def cls_update(st, logits, target, count=None, eps=EPS):
    logits, target = np.asarray(logits), np.asarray(target).reshape(-1)
    count = logits.shape[0] if count is None else count
    _add_rows(st, logits[:count], target[:count], eps)
    return st


def seg_update(st, logits, seg, label, parts, count=None, first=0, eps=EPS):
    """logits [B,P,N], seg [B,N], label [B], parts = (part_start, part_num)."""
    logits, seg, label = np.asarray(logits), np.asarray(seg), np.asarray(label).reshape(-1)
    start, num = (np.asarray(p) for p in parts)
    B, P, N = logits.shape
    count = B if count is None else count
    for b in range(count):
        x = logits[b].T                                       # [N,P]: rows = points
        _add_rows(st, x, seg[b], eps)
        pred = predict(x)
        lab = int(label[b])
        ok = 0 <= lab < len(start) and start[lab] >= 0 and num[lab] >= 1 and start[lab] + num[lab] <= P
        iou = float("nan")
        if ok:
            total = 0.0
            for p in range(int(start[lab]), int(start[lab] + num[lab])):
                inter = int(((pred == p) & (seg[b] == p)).sum())
                union = int(((pred == p) | (seg[b] == p)).sum())
                total += 1.0 if union == 0 else float(inter) / float(union)
            iou = total / float(num[lab])
        st["shape_iou"][first + b] = iou
        st["shape_cat"][first + b] = lab if ok else -2
    return st
