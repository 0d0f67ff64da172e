"""GPU tests (-m gpu) of the feature propagation: svnet_three_nn_f32 / svnet_three_interpolate_f32 (svnet_amd/csrc/propagate.hip)
through svnet_amd.propagate against the numpy restatement tests/propagate_ref.py and the reference's recorded results
(tests/golden/propagate.npz), and train.evaluate_dense against tests/metrics_ref.py.  The contract is single-rounded fp32, so indices
are compared as integers and dist3, weight and out as BIT PATTERNS: there is no tolerance.  Every reference is computed once per
process and shared."""
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR
from tests import propagate_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "propagate.npz"))
F32 = np.float32
_REF = {}


def _tile():
    try:
        from svnet_amd import propagate as Pr
        return Pr.tile()
    except Exception:                 # the library or the module is missing: the tests still fail, at the import in the test
        return 2048


T = _tile()
# (P, N, D) at B = 2: every N in {1, 2, 3, 4, 63, 64, 65, tile - 1, tile, tile + 1, 2 tile + 5}, every P in {1, 63, 64, 65, 257, 1000}
# (partial waves and workgroups of 256) and every D in {1, 2, 50, 65} once, plus the part-segmentation shape.
CASES = [(1, 1, 1), (63, 2, 2), (64, 3, 50), (65, 4, 65), (257, 63, 1), (1000, 64, 2), (65, 65, 50), (257, T - 1, 2), (64, T, 1),
         (63, T + 1, 65), (257, 2 * T + 5, 2), (2500, 2048, 50)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _ref(key, q, r, f):
    """(idx, dist3, weight, out) of the restatement, computed once."""
    if key not in _REF:
        idx, dist3, w = R.three_nn_batch(q, r)
        out = np.stack([R.three_interpolate(f[b], idx[b], w[b]) for b in range(q.shape[0])])
        for a in (idx, dist3, w, out):
            a.setflags(write=False)
        _REF[key] = (idx, dist3, w, out)
    return _REF[key]


def _same_bits(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got, want) if got.dtype == np.int64 else (_bits(got), _bits(want))
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %r: got %r, want %r" % (
        tag, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _run_all(dev, q, r, f):
    """The three public calls on the device; propagate() must equal three_nn + three_interpolate bit for bit."""
    from svnet_amd import propagate as Pr
    tq, tr, tf = (torch.from_numpy(a).to(dev) for a in (q, r, f))
    idx, dist3, w = Pr.three_nn(tq, tr)
    out = Pr.three_interpolate(tf, idx, w)
    both = Pr.propagate(tq, tr, tf)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == q.shape and tuple(out.shape) == (q.shape[0], f.shape[1], q.shape[1])
    assert torch.equal(out.view(torch.int32), both.view(torch.int32))
    return idx.cpu().numpy(), dist3.cpu().numpy(), w.cpu().numpy(), out.cpu().numpy()


def _check_case(dev, key, q, r, f, tag):
    got = _run_all(dev, q, r, f)
    want = _ref(key, q, r, f)
    for g, w, what in zip(got, want, ("idx", "dist3", "weight", "out")):
        _same_bits(g, w, "%s %s" % (tag, what))
    return got


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("P,N,D", CASES, ids=lambda v: str(v))
def test_kernels_equal_the_restatement(P, N, D, kind, hip_device):
    make = R.lattice_case if kind == "lattice" else R.gauss_case
    q, r, f = make(5000 + N, 2, P, N, D)
    idx, dist3, w, _ = _check_case(hip_device, (kind, P, N, D), q, r, f, "%s B 2 P %d N %d D %d" % (kind, P, N, D))
    assert ((idx >= 0) & (idx < N)).all() and (dist3[:, :, :min(3, N)] >= 0).all()
    assert (idx[:, :, min(3, N):] == 0).all() and (w[:, :, min(3, N):] == 0).all()              # slots past K


def test_ties_all_sampled_points_identical(hip_device):
    N = T + 7
    q = R.gauss_case(61, 2, 130, 4, 1)[0]
    r = np.ascontiguousarray(np.tile(np.array([[0.25, -0.5, 0.75]], dtype=F32), (2, N, 1)))
    f = R.gauss_case(61, 2, 130, N, 3)[2]
    idx = _check_case(hip_device, "identical", q, r, f, "identical points")[0]
    assert (idx == np.array([0, 1, 2])).all()


def test_ties_duplicates_across_the_tile_boundary(hip_device):
    """Duplicated sampled points at indices tile - 1 and tile - the last candidate of one LDS tile and the first of the next - and
    every query equal to one of the duplicated points: the pair is at distance 0 and the lower index comes first."""
    N = T + 40
    q, r, f = R.gauss_case(62, 2, 70, N, 2)
    r[:, T] = r[:, T - 1]
    q[:, ::2] = r[:, T - 1:T]                                        # every second query AT the pair
    q, r = np.ascontiguousarray(q), np.ascontiguousarray(r)
    idx, dist3, _, _ = _check_case(hip_device, "boundary", q, r, f, "tile boundary")
    assert (idx[:, ::2, 0] == T - 1).all() and (idx[:, ::2, 1] == T).all() and (dist3[:, ::2, :2] == 0).all()


def test_queries_equal_to_sampled_points(hip_device):
    """What resample_fps produces: every sampled point IS a query.  dist3 is exactly 0 there and the point's own value dominates."""
    q, _, _ = R.gauss_case(63, 2, 600, 4, 1)
    r = np.ascontiguousarray(q[:, 5::4][:, :128])
    f = R.gauss_case(63, 2, 600, 128, 5)[2]
    idx, dist3, w, out = _check_case(hip_device, "coincident", q, r, f, "queries at sampled points")
    own = np.arange(128)
    assert (idx[:, 5 + 4 * own, 0] == own).all() and (dist3[:, 5 + 4 * own, 0] == 0).all() and (dist3 >= 0).all()
    assert (w[:, 5 + 4 * own, 0] > 0.999).all()
    assert abs(out[:, :, 5 + 4 * own] - f).max() < 1e-2


def test_non_finite_coordinates_leave_indices_in_range(hip_device):
    from svnet_amd import propagate as Pr
    q, r, f = R.gauss_case(64, 2, 300, T + 9, 4)
    q[0, 7] = np.nan                       # one NaN query
    q[1, 290, 1] = np.nan
    r[0, 3, 2] = np.inf                    # one infinite sampled point
    r[1, T + 2, 0] = -np.inf
    tq, tr, tf = (torch.from_numpy(np.ascontiguousarray(a)).to(hip_device) for a in (q, r, f))
    idx, _, _ = Pr.three_nn(tq, tr)
    Pr.propagate(tq, tr, tf)
    idx = idx.cpu().numpy()
    assert ((idx >= 0) & (idx < T + 9)).all(), (idx.min(), idx.max())


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_golden_through_the_kernels(name, hip_device):
    q, r, f = GOLDEN[name + "_q"], GOLDEN[name + "_r"], GOLDEN[name + "_f"]
    idx, _, _, out = _run_all(hip_device, q, r, f)
    _same_bits(out, GOLDEN[name + "_out"], "%s out" % name)
    if name + "_idx" in GOLDEN.files:
        _same_bits(idx, GOLDEN[name + "_idx"], "%s idx" % name)


def test_propagate_in_a_captured_graph(hip_device):
    """propagate(out=buf) captured on a side stream after a warm-up; two replays with the inputs refilled in place between them each
    equal the eager result on those inputs bit for bit."""
    from svnet_amd import propagate as Pr
    dev = hip_device
    sets = [R.gauss_case(70 + i, 2, 700, 128, 50) for i in range(2)]
    tq, tr, tf = (torch.from_numpy(a).to(dev) for a in sets[0])
    buf = torch.zeros(2, 50, 700, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        Pr.propagate(tq, tr, tf, out=buf)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = Pr.propagate(tq, tr, tf, out=buf)
    assert res is buf
    for q, r, f in (sets[1], sets[0]):
        tq.copy_(torch.from_numpy(q)); tr.copy_(torch.from_numpy(r)); tf.copy_(torch.from_numpy(f))
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = buf.clone()
        eager = Pr.propagate(tq, tr, tf)
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
        assert float(replayed.abs().max()) > 0


def test_refusals_on_the_device(hip_device):
    from svnet_amd import propagate as Pr
    from svnet_amd._lib import SvnetHipError
    dev = hip_device
    q, r, f = (torch.from_numpy(a).to(dev) for a in R.gauss_case(65, 2, 10, 5, 4))
    with pytest.raises(ValueError):
        Pr.three_nn(q, r.cpu())                                        # mismatched devices
    with pytest.raises(ValueError):
        Pr.propagate(q, r, f, out=torch.empty(2, 4, 11, device=dev))
    with pytest.raises(TypeError):
        Pr.propagate(q, r, f, out=torch.empty(2, 4, 10, device=dev, dtype=torch.float64))
    with pytest.raises(SvnetHipError):
        Pr.three_nn(q, torch.zeros(2, 32769, 3, device=dev))
    with pytest.raises(SvnetHipError):
        Pr.three_nn(q, torch.zeros(2, 0, 3, device=dev))
    with pytest.raises(SvnetHipError):
        Pr.three_interpolate(torch.zeros(2, 0, 5, device=dev), torch.zeros(2, 10, 3, dtype=torch.int64, device=dev), torch.zeros(2, 10, 3, device=dev))
    # an index outside [0, N) is clamped, never followed
    idx = torch.tensor([[[-5, 0, 99]]], dtype=torch.int64, device=dev)
    w = torch.tensor([[[0.5, 0.25, 0.25]]], device=dev)
    feat = torch.tensor([[[1.0, 2.0, 4.0]]], device=dev)
    assert float(Pr.three_interpolate(feat, idx, w)) == 0.5 * 1.0 + 0.25 * 1.0 + 0.25 * 4.0


# ---- the resampled pool: source_points and evaluate_dense
M_POOL, P_POOL, N_POOL, PARTS = 5, 700, 128, 50


def _pools(dev):
    from svnet_amd.data import DevicePool
    dense = DevicePool.synthetic(81, M_POOL, P_POOL, 16, PARTS, device=dev)
    return dense, dense.resample_fps(N_POOL, seed=2, normalize=True)


def test_source_points(hip_device):
    from svnet_amd import propagate as Pr
    from svnet_amd.data import DevicePool
    dense, pool = _pools(hip_device)
    want = torch.gather(dense.data, 1, pool.fps_index.unsqueeze(2).expand(-1, -1, 3))
    for got in (Pr.source_points(pool, dense), pool.source_points(dense)):
        assert got.is_contiguous() and tuple(got.shape) == (M_POOL, N_POOL, 3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(pool.data, want)                                   # normalize=True moved the pool's own coordinates
    with pytest.raises(ValueError):
        Pr.source_points(dense, dense)                                        # no fps_index
    with pytest.raises(ValueError):
        Pr.source_points(pool, DevicePool.synthetic(81, M_POOL + 1, P_POOL, 16, PARTS, device=hip_device))
    with pytest.raises(ValueError):
        Pr.source_points(pool, DevicePool.synthetic(81, M_POOL, 100, 16, PARTS, device=hip_device))     # fewer points than sampled


class _StandInStep:
    """The ForwardStep protocol (run() / out) without a model: logits [B,50,N] = a fixed, seeded affine function of loader.x [B,3,N],
    computed with torch operations; every batch's logits are kept ON THE DEVICE for the test's own reference."""

    def __init__(self, loader):
        from svnet_amd import synth
        dev = loader.x.device
        self.loader = loader
        self.W = torch.from_numpy(synth.normal(82, 0, (PARTS, 3))).to(dev)
        self.b = torch.from_numpy(synth.normal(82, 1, (PARTS, 1))).to(dev)
        self.out, self.kept = None, []

    def run(self):
        self.out = (torch.einsum("cd,bdn->bcn", self.W, self.loader.x) * 3.0 + self.b).contiguous()
        self.kept.append(self.out.clone())
        return self.out


def _loader(pool, **kw):
    from svnet_amd.data import BatchLoader
    args = dict(select="first_ordered", scale_shift=False, rotate="none", shuffle=False, drop_last=False, seed=1)
    args.update(kw)
    return BatchLoader(pool, 2, N_POOL, **args)


def test_evaluate_dense_end_to_end(hip_device):
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    from svnet_amd.train import evaluate_dense
    dense, pool = _pools(hip_device)
    loader = _loader(pool)
    assert len(loader) == 3                                                   # 2 + 2 + 1: a short last batch
    step = _StandInStep(loader)
    metrics = EpochMetrics(PARTS, hip_device, parts=SHAPENET_PARTS, capacity=M_POOL)
    result = evaluate_dense(step, loader, metrics, dense)
    state = metrics.state()

    data, seg, label = dense.data.cpu().numpy(), dense.seg.cpu().numpy(), dense.label.cpu().numpy()
    fps = pool.fps_index.cpu().numpy()
    want, bound = MR.new_state(PARTS, M_POOL), 0.0
    for i, kept in enumerate(step.kept):
        first, count = 2 * i, min(2, M_POOL - 2 * i)
        logits = kept.cpu().numpy()[:count]
        sl = slice(first, first + count)
        ref = np.stack([data[m, fps[m]] for m in range(first, first + count)])
        up = R.propagate_batch(data[sl], ref, logits)                         # [count,50,P] on the dense clouds
        MR.seg_update(want, up, seg[sl], label[sl], SHAPENET_PARTS, count, first)
        bound += MR.loss_bound(up.transpose(0, 2, 1).reshape(-1, PARTS), seg[sl].reshape(-1))
    assert len(step.kept) == 3
    assert np.array_equal(state["conf"], want["conf"]) and state["rows"] == want["rows"] == M_POOL * P_POOL
    assert state["invalid"] == want["invalid"] == 0
    assert np.array_equal(state["shape_cat"], want["shape_cat"]) and (state["shape_cat"] >= 0).all()
    assert np.array_equal(state["shape_iou"].view(np.int64), want["shape_iou"].view(np.int64))
    err = abs(state["loss_sum"] - want["loss_sum"])
    print("evaluate_dense: loss_sum %.9f, |error| %.3e of bound %.3e" % (state["loss_sum"], err, bound))
    assert err <= bound, (err, bound)
    rw = EpochMetrics.finalize(want)
    assert result == EpochMetrics.finalize(state)
    for key in ("acc", "balanced_acc", "rows", "invalid", "shape_iou", "class_iou", "shapes"):
        assert result[key] == rw[key], key
    assert result["shapes"] == M_POOL and result["rows"] == M_POOL * P_POOL


def test_evaluate_dense_refuses_loaders_that_reorder(hip_device):
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    from svnet_amd.train import evaluate_dense
    dense, pool = _pools(hip_device)
    metrics = EpochMetrics(PARTS, hip_device, parts=SHAPENET_PARTS, capacity=M_POOL)
    for kw in (dict(shuffle=True), dict(select="first_shuffled"), dict(drop_last=True)):
        loader = _loader(pool, **kw)
        with pytest.raises(ValueError):
            evaluate_dense(_StandInStep(loader), loader, metrics, dense)
    loader = _loader(dense.resample_fps(N_POOL, seed=2))
    loader.pool.fps_index = None                                              # a pool that was not resampled
    with pytest.raises(ValueError):
        evaluate_dense(_StandInStep(loader), loader, metrics, dense)
    loader = _loader(pool)
    with pytest.raises(ValueError):
        evaluate_dense(_StandInStep(loader), loader, EpochMetrics(PARTS, hip_device, parts=SHAPENET_PARTS, capacity=M_POOL - 1), dense)
