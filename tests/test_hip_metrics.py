"""GPU tests (-m gpu) of the epoch metrics: svnet_metrics_cls_f32 / svnet_metrics_seg_f32 (svnet_amd/csrc/metrics.hip) through
svnet_amd.metrics.EpochMetrics against the numpy restatement tests/metrics_ref.py (itself pinned to the reference's recorded results
by tests/test_host_metrics.py), and train_epoch(..., metrics=) / evaluate on top of captured steps.

Integers (confusion matrix, rows, invalid) and the float64 shape IoUs must be EQUAL.  The loss sum is fp32 work per row: it is held
to metrics_ref.loss_bound, the worst case of that arithmetic derived operation by operation from the inputs (no margin on top: every
term of it already counts a full ulp where the operation's error is half of one); every case prints its error next to its bound."""
import argparse
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR

pytestmark = pytest.mark.gpu

SEED = 91
# a second part table (3 categories over 70 parts) for the tier of the seg kernel above 64 channels
PARTS70 = ((0, 20, 64), (20, 44, 6))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_state(got, want, tag, loss_bound=None):
    assert np.array_equal(got["conf"], want["conf"]), tag
    assert got["rows"] == want["rows"] and got["invalid"] == want["invalid"], (tag, got["rows"], want["rows"], got["invalid"], want["invalid"])
    assert int(got["conf"].sum()) == got["rows"], tag
    if "shape_cat" in want:
        assert np.array_equal(got["shape_cat"], want["shape_cat"]), tag
        same = _bits(got["shape_iou"]) == _bits(want["shape_iou"])
        nan = np.isnan(got["shape_iou"]) & np.isnan(want["shape_iou"])
        assert (same | nan).all(), (tag, np.argwhere(~(same | nan))[:4])
    if loss_bound is not None:
        err = abs(got["loss_sum"] - want["loss_sum"])
        print("%s: loss_sum %.9f, |error| %.3e of bound %.3e (%d rows)" % (tag, got["loss_sum"], err, loss_bound, got["rows"]))
        assert err <= loss_bound, (tag, err, loss_bound)


def _quantised(rng, shape):
    """Logits on a grid of 0.5: exact ties for the maximum are common."""
    return (np.round(rng.standard_normal(shape) * 4.0) / 2.0).astype(np.float32)


@pytest.mark.parametrize("C", [2, 40, 65])
@pytest.mark.parametrize("R", [1, 32, 4097])
def test_cls_update_equals_the_restatement(R, C, hip_device):
    from svnet_amd.metrics import EpochMetrics
    rng = np.random.default_rng(1000 * R + C)
    x = _quantised(rng, (R, C))
    y = rng.integers(0, C, R)
    assert ((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).any() or R == 1
    m = EpochMetrics(C, hip_device)
    # ---- integers: ties, and (R > 1) a NaN row, targets out of range, count < R
    xi, yi = x.copy(), y.copy()
    count = R
    if R > 1:
        xi[1, C // 2:] = np.nan                               # the first NaN is the row's maximum
        yi[[0, R // 2]] = [-1, C]
        xi[R - 1, :] = np.nan
        yi[R - 1] = -7                                        # (rows past `count`, and invalid rows, are never read as an index)
        count = R - R // 3 if R > 32 else R
    m.update(torch.from_numpy(xi).to(hip_device), torch.from_numpy(yi).to(hip_device), count)
    got, want = m.state(), MR.cls_update(MR.new_state(C), xi, yi, count)
    _same_state(got, want, "cls integers R %d C %d" % (R, C))
    if R > 1:
        assert want["invalid"] >= 1 and np.isnan(got["loss_sum"]) == np.isnan(want["loss_sum"])
        assert got["conf"][yi[1], C // 2] >= 1
    # ---- loss on finite rows; two passes: the same bits; accumulation over two updates
    xc = (x + rng.standard_normal((R, C)).astype(np.float32)).astype(np.float32)
    dx, dy = torch.from_numpy(xc).to(hip_device), torch.from_numpy(y).to(hip_device)
    passes = []
    for _ in range(2):
        m.reset()
        m.update(dx, dy)
        m.update(dx, dy, R)
        passes.append(m.state())
    want = MR.cls_update(MR.cls_update(MR.new_state(C), xc, y), xc, y)
    _same_state(passes[0], want, "cls loss R %d C %d" % (R, C), loss_bound=2 * MR.loss_bound(xc, y))      # (the rows were added twice)
    assert _bits(passes[0]["loss_sum"]) == _bits(passes[1]["loss_sum"]) and np.array_equal(passes[0]["conf"], passes[1]["conf"])
    r = EpochMetrics.finalize(passes[0])
    assert r["rows"] == 2 * R and abs(r["acc"] - float((MR.predict(xc) == y).mean())) < 1e-15


def _seg_inputs(rng, B, P, N, parts):
    start, num = (np.asarray(p) for p in parts)
    label = rng.integers(0, len(start), B)
    seg = np.stack([start[c] + rng.integers(0, num[c], N) for c in label]).astype(np.int64)
    x = _quantised(rng, (B, P, N))
    hit = rng.random((B, N)) < 0.6
    bi, ni = np.nonzero(hit)
    x[bi, seg[bi, ni], ni] += 3.0
    return x, seg, label.astype(np.int64)


@pytest.mark.parametrize("shape", [(2, 50, 100), (32, 50, 2048), (3, 70, 300), (5, 2, 64)], ids=lambda s: "B%d_P%d_N%d" % s)
def test_seg_update_equals_the_restatement(shape, hip_device):
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    B, P, N = shape
    parts = SHAPENET_PARTS if P == 50 else PARTS70 if P == 70 else ((0,), (2,))
    rng = np.random.default_rng(7 * B + P + N)
    x, seg, label = _seg_inputs(rng, B, P, N, parts)
    cap = B + 5
    # poison: the loader's (label -1, every point -1) in the last cloud, stray out-of-range points, a label past the table
    seg[B - 1, :] = -1
    label[B - 1] = -1
    seg[0, [3, N - 1]] = [P, -3]
    if B > 2:
        label[1] = len(parts[0])
    dev = [torch.from_numpy(a).to(hip_device) for a in (x, seg, label)]
    for count, first in ((B, 2), (max(1, B - 1), 0)) if B > 2 else ((B, 2), (1, 4)):
        tag = "seg B %d P %d N %d count %d first %d" % (B, P, N, count, first)
        passes = []
        for _ in range(2):
            m = EpochMetrics(P, hip_device, parts=parts, capacity=cap)
            m.update(dev[0], dev[1], count, label=dev[2], first=first)
            passes.append(m.state())
        want = MR.seg_update(MR.new_state(P, cap), x, seg, label, parts, count, first)
        ok = (seg[:count] >= 0) & (seg[:count] < P)
        rows = x[:count].transpose(0, 2, 1)[ok]
        _same_state(passes[0], want, tag, loss_bound=MR.loss_bound(rows, seg[:count][ok]))
        assert want["invalid"] >= 2 and (want["shape_cat"] == -1).sum() == cap - count
        if count == B:
            assert want["shape_cat"][first + B - 1] == -2 and np.isnan(passes[0]["shape_iou"][first + B - 1])
        assert _bits(passes[0]["loss_sum"]) == _bits(passes[1]["loss_sum"])
    # first + count past the capacity is refused on the host, and nothing was written
    from svnet_amd._lib import SvnetHipError
    with pytest.raises(SvnetHipError, match="capacity"):
        m.update(dev[0], dev[1], B, label=dev[2], first=cap - B + 1)
    m.reset()
    empty = m.state()
    assert empty["rows"] == 0 and empty["conf"].sum() == 0 and (empty["shape_cat"] == -1).all() and np.isnan(empty["shape_iou"]).all()


# ----------------------------------------------------------------------------- end to end: captured steps over synthetic pools

def _cls_model(dev, k=8):
    import svnet_amd.models as M
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return M.SV_DGCNN_CLS(argparse.Namespace(k=k, binary=True), 40).to(dev).train()


def _seg_model(dev, k=8):
    import svnet_amd.models as M
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return M.SV_DGCNN_PSEG(argparse.Namespace(k=k, binary=True, dropout=0.0), 50).to(dev).train()


# fwd + bwd of one step from the SAME parameters twice: the losses are bit-identical, the gradients agree to the order of the float
# atomics in the weight-gradient reductions (~1e-5 of the bucket's largest entry); 1e-3 is the tolerance the
# project holds gradients to everywhere (smoke, the parity suites)
GRAD_NOISE = 1e-3


def _train_once(kind, dev, with_metrics, replay=None):
    """One epoch (3 captured steps of B = 4, N = 128, eager FlatAdam) from seeded parameters.

    Two free-running epochs of the SAME code do not end in the same bits here - with or without metrics: the weight-gradient
    reductions add with float atomics, and a binarized net under Adam amplifies a last-bit difference (tests/test_hip_graph.py says
    the same of its optimizer test) - so "with metrics" against "without" as two free runs would measure that noise, not the metrics.
    The noise is therefore taken out where it enters: `replay` = the per-step gradient buckets recorded by an earlier run are written
    over this run's own gradients (after the real step ran, and after checking that they agree to GRAD_NOISE) before anything else
    reads them.  Everything else - forward, loss, BatchNorm statistics, optimizer, re-packing, the metrics launch - is deterministic,
    so from then on the two epochs must agree bit for bit: parameters, optimizer moments and every step's loss.
    Returns a dict: flat, m, v (clones), mean, losses, grads, state, seen, loader."""
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    from svnet_amd.train import FlatAdam, FlatParams, TrainStep, seg_loss, train_epoch
    seg = kind == "seg"
    pool = DevicePool.synthetic(21, 13, 256, 16 if seg else 40, 50 if seg else None, device=dev)
    loader = BatchLoader(pool, 4, 128, select="first_shuffled", scale_shift=True, rotate="z", seed=SEED, num_cat=16 if seg else None)
    model = _seg_model(dev) if seg else _cls_model(dev)
    fp = FlatParams(model)
    if seg:
        step = TrainStep(model, (loader.x, loader.onehot), loader.seg, loss_fn=seg_loss, keep_output=with_metrics)
    else:
        step = TrainStep(model, (loader.x,), loader.y, keep_output=with_metrics)
    loader.load(0)
    step.capture()
    opt = FlatAdam(fp, step.bucket, lr=1e-3)
    metrics = (EpochMetrics(50, dev, parts=SHAPENET_PARTS, capacity=pool.M) if seg else EpochMetrics(40, dev)) if with_metrics else None
    seen, grads, losses, noise = [], [], [], []

    class Spy:
        out = None

        def run(self):
            loss = step.run()
            losses.append(loss.clone())
            if replay is not None:
                theirs = replay[len(grads)]
                noise.append(float((step.bucket.flat - theirs).abs().max() / theirs.abs().max()))
                step.bucket.flat.copy_(theirs)
            grads.append(step.bucket.flat.clone())
            if with_metrics:
                Spy.out = step.out
                seen.append(tuple(t.clone() for t in (step.out, loader.seg if seg else loader.y, loader.y)))
            return loss
    loader.set_epoch(1)
    mean = train_epoch(Spy(), loader, opt, metrics=metrics) if with_metrics else train_epoch(Spy(), loader, opt)
    torch.cuda.synchronize()
    assert opt.steps == 3 and len(loader) == 3
    if replay is not None:
        print("%s: own gradients against the replayed ones, per step (relative to the largest entry): %s" % (kind, " ".join("%.2e" % v for v in noise)))
        assert max(noise) <= GRAD_NOISE, noise
    return dict(flat=fp.flat.clone(), m=opt.m.clone(), v=opt.v.clone(), mean=mean, losses=[float(v) for v in losses], grads=grads,
                state=metrics.state() if with_metrics else None, seen=seen, loader=loader)


def _restate(kind, seen, spans, capacity):
    from svnet_amd.metrics import SHAPENET_PARTS
    st = MR.new_state(50 if kind == "seg" else 40, capacity if kind == "seg" else None)
    bound = 0.0
    for (out, tgt, lab), (first, count) in zip(seen, spans):
        out, tgt, lab = (t.cpu().numpy() for t in (out, tgt, lab))
        if kind == "seg":
            MR.seg_update(st, out, tgt, lab, SHAPENET_PARTS, count, first)
            bound += MR.loss_bound(out[:count].transpose(0, 2, 1).reshape(-1, 50), tgt[:count].reshape(-1))
        else:
            MR.cls_update(st, out, tgt, count)
            bound += MR.loss_bound(out[:count], tgt[:count])
    return st, bound


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_train_epoch_with_metrics(kind, hip_device):
    """train_epoch(..., metrics=) on a captured TrainStep(keep_output=True): the state equals the restatement applied to the per-step
    logits the test collects itself, the returned mean loss is the epoch's loss, and the parameters (and Adam moments, and every
    step's loss) after the epoch are bit-identical to an epoch without metrics - both epochs on the same per-step gradients, see
    _train_once for why and how."""
    from svnet_amd.metrics import EpochMetrics
    base = _train_once(kind, hip_device, False)
    with_m = _train_once(kind, hip_device, True, replay=base["grads"])
    state, seen, loader = with_m["state"], with_m["seen"], with_m["loader"]
    assert len(seen) == 3
    want, bound = _restate(kind, seen, [loader.span(i) for i in range(3)], loader.pool.M)
    _same_state(state, want, "train_epoch %s" % kind, loss_bound=bound)
    r, rw = EpochMetrics.finalize(state), EpochMetrics.finalize(want)
    assert r["rows"] == (12 * 128 if kind == "seg" else 12) and r["invalid"] == 0
    assert r["acc"] == rw["acc"] and r["balanced_acc"] == rw["balanced_acc"]
    if kind == "seg":
        assert r["shape_iou"] == rw["shape_iou"] and r["class_iou"] == rw["class_iou"] and r["shapes"] == 12
    # train_epoch's own mean of the steps' fp32 losses is the same quantity (equal batch sizes): fp32 rounding of each step's mean
    assert abs(with_m["mean"] - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"])), (with_m["mean"], r["loss"])
    assert with_m["losses"] == base["losses"] and with_m["mean"] == base["mean"], (with_m["losses"], base["losses"])
    for key in ("flat", "m", "v"):
        assert torch.equal(with_m[key].view(torch.int32), base[key].view(torch.int32)), "the metrics launch changed the training trajectory: " + key
    assert len(set(base["losses"])) == 3 and not torch.equal(base["grads"][0], base["grads"][1])      # (three real, different steps)


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_evaluate(kind, hip_device):
    """evaluate on a captured ForwardStep over a pool with a short final batch: finalize of the restatement on the logits the test
    spies, and the predictions of eval_epoch on the same pool."""
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    from svnet_amd.train import ForwardStep, eval_epoch, evaluate
    seg = kind == "seg"
    dev = hip_device
    pool = DevicePool.synthetic(22, 10, 256, 16 if seg else 40, 50 if seg else None, device=dev)
    ev = BatchLoader(pool, 4, 128, select="first_ordered", scale_shift=False, rotate="none", shuffle=False, drop_last=False, seed=SEED,
                     num_cat=16 if seg else None)
    assert len(ev) == 3 and ev.span(2) == (8, 2)
    model = _seg_model(dev) if seg else _cls_model(dev)
    ev.load(0)
    fwd = ForwardStep(model, (ev.x, ev.onehot) if seg else (ev.x,)).capture()
    metrics = EpochMetrics(50, dev, parts=SHAPENET_PARTS, capacity=pool.M) if seg else EpochMetrics(40, dev)
    seen = []

    class Spy:
        def run(self):
            out = fwd.run()
            seen.append(tuple(t.clone() for t in (out, ev.seg if seg else ev.y, ev.y)))
            return out
    metrics.update(fwd.run(), ev.seg if seg else ev.y, 4, label=ev.y)
    result = evaluate(Spy(), ev, metrics)                     # (evaluate resets: the update above leaves no trace)
    state = metrics.state()
    want, bound = _restate(kind, seen, [ev.span(i) for i in range(3)], pool.M)
    _same_state(state, want, "evaluate %s" % kind, loss_bound=bound)
    assert result == EpochMetrics.finalize(state)
    rw = EpochMetrics.finalize(want)
    for key in ("acc", "balanced_acc", "rows", "invalid") + (("shape_iou", "class_iou", "shapes") if seg else ()):
        assert result[key] == rw[key], key
    assert result["rows"] == (10 * 128 if seg else 10) and result["invalid"] == 0
    # eval_epoch on the same pool: the same predictions, hence the same confusion matrix
    logits, pred = eval_epoch(fwd, ev)
    truth = (pool.seg[:, :128] if seg else pool.label).cpu().numpy().reshape(-1)
    pred = pred.cpu().numpy().reshape(-1)
    conf = np.zeros_like(state["conf"])
    np.add.at(conf, (truth, pred), 1)
    assert np.array_equal(conf, state["conf"])
    assert abs(result["acc"] - float((truth == pred).mean())) < 1e-15
