"""GPU tests (-m gpu) of the gradients of grouping and interpolation: svnet_pointset_reverse_i32, svnet_three_interpolate_bwd_f32 and
svnet_group_points_bwd_f32 (svnet_amd/csrc/pointset_grad.hip) through svnet_amd.propagate, svnet_amd.group and their autograd
functions, against the numpy restatement tests/pointset_grad_ref.py and the reference's recorded gradients
(tests/golden/pointset_grad.npz); and the modules of svnet_amd/models/utils/pointnet_util.py against the reference's recorded stack.
The sums have a fixed order, so lists are compared as integers and gradients as BIT PATTERNS: there is no tolerance except where a
test says so and derives it.  Every case runs at B = 2; every reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import group_ref as G
from tests import pointset_grad_ref as PG
from tests import propagate_ref as R
from tests.common import compare_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "pointset_grad.npz"))
GROUP_GOLDEN = np.load(os.path.join(HERE, "golden", "group.npz"))
F32 = np.float32
B = 2
_REF = {}


def _thresholds():
    try:
        from svnet_amd import _pointset
        return _pointset.reverse_tile(), _pointset.reverse_chunk()
    except Exception:                 # the library or the names are missing: the tests still fail, at the import in the test
        return 256, 2048


T, CH = _thresholds()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same_bits(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got, want) if got.dtype != F32 else (_bits(got), _bits(want))
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %r: got %r, want %r" % (
        tag, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _once(key, make):
    if key not in _REF:
        res = make()
        for a in (res if isinstance(res, tuple) else (res,)):
            a.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.array(a, order="C")).to(dev) for a in arrays)           # a copy: the shared references are read-only


def _nan_like(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ---- reverse lists.  (R, K, N, kind): N in {1, 2, 3, 64, 65, tile, tile + 1, 2 tile + 5} (one wave, two waves, one and two
# workgroups), R K on both sides of the edge chunk and of a wave's 64-edge step; kinds: seeded targets, targets outside [0, N)
# (clamped), fewer edges than points (empty lists), a hub that takes every edge (list lengths past the chunk), two hubs.
REVERSE_CASES = [(1, 1, 1, "rand"), (5, 3, 2, "rand"), (21, 3, 3, "outside"), (22, 3, 3, "rand"), (700, 3, 64, "rand"), (4, 16, 64, "hub"),
                 (40, 16, 65, "rand"), (3, 3, 65, "rand"), (63, 1, 65, "hub"), (CH // 16, 16, T, "rand"), (CH // 16, 16, T + 1, "hub"),
                 (CH + 1, 1, 64, "hub"), (CH - 1, 1, T + 1, "rand"), (CH // 3 + 1, 3, T + 1, "outside"), (2 * CH // 3 + 30, 3, 2 * T + 5, "two"),
                 (9, 3, T + 1, "rand"), (1000, 8, 3000, "rand")]


def _table(R_, K, N, kind):
    seed = 7000 + R_ + 31 * K + N
    if kind == "rand":
        idx = synth.integers(seed, 1, (B, R_, K), N)
    elif kind == "outside":
        idx = synth.integers(seed, 1, (B, R_, K), N + 10) - 5
    elif kind == "hub":
        idx = np.full((B, R_, K), N - 1, dtype=np.int64)
        idx[1] = 0
    else:                                                            # two hubs, the first and the last point, alternating edges
        idx = np.zeros((B, R_, K), dtype=np.int64)
        idx.reshape(B, -1)[:, ::2] = N - 1
    return np.ascontiguousarray(idx.astype(np.int64))


@pytest.mark.parametrize("R_,K,N,kind", REVERSE_CASES, ids=lambda v: str(v))
def test_reverse_lists_equal_the_restatement(R_, K, N, kind, hip_device):
    from svnet_amd import _pointset
    idx = _table(R_, K, N, kind)
    want_start, want_edge = _once(("rev", R_, K, N, kind), lambda: PG.reverse_lists_batch(idx, N))
    if R_ * K < N:
        assert (np.diff(want_start, axis=1) == 0).any()              # empty lists are in
    start, edge = _pointset.reverse_lists(_dev(hip_device, idx)[0], N)
    assert start.dtype == torch.int32 and tuple(start.shape) == (B, N + 1) and edge.dtype == torch.int32 and tuple(edge.shape) == (B, R_ * K)
    _same_bits(start.cpu().numpy(), want_start, "rev_start")
    _same_bits(edge.cpu().numpy(), want_edge, "rev_edge")
    again = _pointset.reverse_lists(_dev(hip_device, idx)[0], N)
    assert torch.equal(again[0], start) and torch.equal(again[1], edge)


# ---- interpolation backward
INTERP_CASES = [(1, 1, 1), (63, 2, 2), (65, 3, 50), (257, 65, 65), (1000, 64, 1), (64, T + 1, 2)]


def _interp_inputs(kind, P, N, D):
    if kind == "one_point":                                          # all queries at one sampled point: a hub of P edges
        q, r, f = R.gauss_case(5100 + N, B, P, N, D)
        q[:] = r[:, 7:8]
    else:
        q, r, f = (R.lattice_case if kind == "lattice" else R.gauss_case)(5100 + N, B, P, N, D)
    dout = synth.normal(5100 + N, 5, (B, D, P))
    return np.ascontiguousarray(q), r, f, dout


def _interp_ref(kind, P, N, D):
    def make():
        q, r, f, dout = _interp_inputs(kind, P, N, D)
        idx, _, w = R.three_nn_batch(q, r)
        return idx, w, PG.interpolate_bwd_batch(dout, idx, w, N)
    return _once(("interp", kind, P, N, D), make)


def _check_interp(dev, kind, P, N, D):
    from svnet_amd import propagate as Pr
    q, r, f, dout = _interp_inputs(kind, P, N, D)
    idx, w, want = _interp_ref(kind, P, N, D)
    tq, tr, tf, tg, ti, tw = _dev(dev, q, r, f, dout, idx, w)
    tag = "%s P %d N %d D %d" % (kind, P, N, D)
    buf = _nan_like((B, D, N), dev)                                  # an unwritten element would stay NaN
    got = Pr.three_interpolate_backward(tg, ti, tw, N, out=buf)
    assert got is buf
    _same_bits(got.cpu().numpy(), want, tag + " three_interpolate_backward")
    _same_bits(Pr.three_interpolate_backward(tg, ti, tw, N).cpu().numpy(), want, tag + " second run")
    plain = Pr.propagate(tq, tr, tf)
    for call in (lambda x: Pr.propagate(tq, tr, x), lambda x: Pr.three_interpolate(x, ti, tw)):
        leaf = tf.clone().requires_grad_()
        out = call(leaf)
        assert out.requires_grad and torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))     # the forward's bits do not change
        out.backward(tg)
        _same_bits(leaf.grad.cpu().numpy(), want, tag + " .backward()")
    return want


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("P,N,D", INTERP_CASES, ids=lambda v: str(v))
def test_interpolation_backward_equals_the_restatement(P, N, D, kind, hip_device):
    _check_interp(hip_device, kind, P, N, D)


def test_interpolation_backward_all_queries_at_one_sampled_point(hip_device):
    want = _check_interp(hip_device, "one_point", 300, 20, 3)
    idx = _interp_ref("one_point", 300, 20, 3)[0]
    assert (idx[:, :, 0] == 7).all() and (want[:, :, 7] != 0).all()


# ---- grouping backward.  Radius 4 takes every point (full groups), 0.3 leaves partial ones; planted centres far outside give empty groups.
GROUP_CASES = [(1, 1, 1, 1), (65, 7, 1, 5), (64, 64, 64, 1), (300, 33, 8, 61), (T + 1, 40, 16, 64)]


def _group_inputs(kind, N, S, nsample, D, radius):
    x, c, pts = (G.lattice_case if kind == "lattice" else G.gauss_case)(6100 + N, B, N, S, D)
    if S >= 7:
        c[:, 2] = 9.0                                                # planted: no point within any radius used here
        c[1, 5] = -9.0
    g = synth.normal(6100 + N, 6, (B, S, nsample, 3 + D))
    return x, np.ascontiguousarray(c), pts, g, G.r2_of(radius)


def _group_ref(kind, N, S, nsample, D, radius):
    def make():
        x, c, _, g, r2 = _group_inputs(kind, N, S, nsample, D, radius)
        idx, count = G.query_ball_batch(x, c, r2, nsample)
        return idx, count, PG.group_bwd_batch(g, idx, N)
    return _once(("group", kind, N, S, nsample, D, radius), make)


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("radius", [0.3, 4.0])
@pytest.mark.parametrize("N,S,nsample,D", GROUP_CASES, ids=lambda v: str(v))
def test_grouping_backward_equals_the_restatement(N, S, nsample, D, radius, kind, hip_device):
    from svnet_amd import group as Gr
    dev = hip_device
    x, c, pts, g, _ = _group_inputs(kind, N, S, nsample, D, radius)
    idx, count, want = _group_ref(kind, N, S, nsample, D, radius)
    if S >= 7:
        assert (count[:, 2] == 0).all() and count[1, 5] == 0 and (idx[:, 2] == 0).all()          # the empty groups are in
    if radius == 4.0:
        assert (count[:, :2] == nsample).all()
    elif N >= 300:
        assert ((count > 0) & (count < nsample)).any()
    tx, tc, tp, tg, ti = _dev(dev, x, c, pts, g, idx)
    tag = "%s N %d S %d nsample %d D %d radius %g" % (kind, N, S, nsample, D, radius)
    buf = _nan_like((B, N, D), dev)
    got = Gr.group_points_backward(tg, ti, N, out=buf)
    assert got is buf
    _same_bits(got.cpu().numpy(), want, tag + " group_points_backward")
    _same_bits(Gr.group_points_backward(tg, ti, N).cpu().numpy(), want, tag + " second run")
    plain = Gr.group_points(tx, tc, ti, tp)
    leaf = tp.clone().requires_grad_()
    out = Gr.group_points(tx, tc, ti, leaf)
    assert out.requires_grad and torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))
    out.backward(tg)
    _same_bits(leaf.grad.cpu().numpy(), want, tag + " .backward()")


def test_sample_and_group_carries_the_gradient(hip_device):
    """sample_and_group and sample_and_group_all with points that require grad: the same bits as the calls without, and the
    gradient of group_points_backward on the indices the call used."""
    from svnet_amd import group as Gr
    dev = hip_device
    x, _, pts = G.lattice_case(6200, B, 300, 4, 6)
    tx, tp = _dev(dev, x, pts)
    start = torch.tensor([3, 250], dtype=torch.int64, device=dev)
    new_xyz, plain = Gr.sample_and_group(32, 0.3, 8, tx, tp, start=start)
    leaf = tp.clone().requires_grad_()
    new_xyz2, out = Gr.sample_and_group(32, 0.3, 8, tx, leaf, start=start)
    assert out.requires_grad and not new_xyz2.requires_grad
    assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32)) and torch.equal(new_xyz, new_xyz2)
    g = _dev(dev, synth.normal(6200, 6, (B, 32, 8, 9)))[0]
    out.backward(g)
    idx = Gr.query_ball_point(0.3, 8, tx, new_xyz)
    want = PG.group_bwd_batch(g.cpu().numpy(), idx.cpu().numpy(), 300)
    _same_bits(leaf.grad.cpu().numpy(), want, "sample_and_group .backward()")
    leaf = tp.clone().requires_grad_()
    _, every = Gr.sample_and_group_all(tx, leaf)
    ga = _dev(dev, synth.normal(6200, 7, (B, 1, 300, 9)))[0]
    every.backward(ga)
    _same_bits(leaf.grad.cpu().numpy(), ga[:, 0, :, 3:].cpu().numpy(), "sample_and_group_all .backward()")


# ---- the reference's recorded gradients
@pytest.mark.parametrize("name", PG.GROUP_CASES)
def test_golden_grouping_gradient_bit_for_bit(name, hip_device):
    from svnet_amd import group as Gr
    N = G.GOLDEN_CASES[name][2]
    x, pts, idx, c = (GROUP_GOLDEN[name + s] for s in ("_xyz", "_points", "_idx", "_new_xyz"))
    tx, tc, tp, ti, tg = _dev(hip_device, x, c, pts, idx, GOLDEN["ga_%s_g" % name].astype(F32))
    want = GOLDEN["ga_%s_dpoints" % name]
    _same_bits(Gr.group_points_backward(tg, ti, N).cpu().numpy(), want, name + " group_points_backward")
    leaf = tp.clone().requires_grad_()
    Gr.group_points(tx, tc, ti, leaf).backward(tg)
    _same_bits(leaf.grad.cpu().numpy(), want, name + " .backward()")


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_golden_interpolation_gradient_within_the_bound(name, hip_device):
    from svnet_amd import propagate as Pr
    seed, Bc, P, N, D = R.GOLDEN_CASES[name]
    q, r, f = R.lattice_case(seed, Bc, P, N, D)
    dout, want = GOLDEN["gb_%s_dout" % name], GOLDEN["gb_%s_dfeat" % name]
    tq, tr, tf, tg = _dev(hip_device, q, r, f, dout)
    idx, _, w = Pr.three_nn(tq, tr)
    leaf = tf.clone().requires_grad_()
    Pr.propagate(tq, tr, leaf).backward(tg)
    got = leaf.grad.cpu().numpy()
    _same_bits(Pr.three_interpolate_backward(tg, idx, w, N).cpu().numpy(), got, name + " functional against .backward()")
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    for b in range(Bc):
        exact, bound = PG.interpolate_bwd_f64(dout[b], idx[b], w[b], N)
        err, off = np.abs(got[b] - exact), np.abs(got[b].astype(np.float64) - want[b])
        print("%s cloud %d: |got - f64| at most %.3f of the bound, |got - reference| %.3f" % (
            name, b, float((err / np.maximum(bound, 1e-300)).max()), float((off / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all() and (off <= bound).all(), name


# ---- the adjoint identity <fwd(f), g> = <f, bwd(g)>, both sides evaluated in float64 from the device's fp32 results
def test_adjoint_identity_of_the_interpolation(hip_device):
    from svnet_amd import propagate as Pr
    P, N, D = 257, 65, 65
    q, r, f, g = _interp_inputs("gauss", P, N, D)
    idx, w, _ = _interp_ref("gauss", P, N, D)
    tf, tg, ti, tw = _dev(hip_device, f, g, idx, w)
    fwd = Pr.three_interpolate(tf, ti, tw).cpu().numpy().astype(np.float64)
    bwd = Pr.three_interpolate_backward(tg, ti, tw, N).cpu().numpy().astype(np.float64)
    lhs, rhs, bound = float((fwd * g).sum()), float((f.astype(np.float64) * bwd).sum()), 0.0
    for b in range(B):
        # the forward's bound is the same statement with lists of length 3: 3 * 2^-23 * sum_j |f_j w_j| per output
        mag = (np.abs(f[b].astype(np.float64))[:, idx[b]] * np.abs(w[b].astype(np.float64))[None]).sum(axis=2)
        bound += float((np.abs(g[b]) * 3 * 2.0 ** -23 * mag).sum())
        bound += float((np.abs(f[b]) * PG.interpolate_bwd_f64(g[b], idx[b], w[b], N)[1]).sum())
    print("interpolation: <fwd(f), g> %.9f, <f, bwd(g)> %.9f, difference %.3e of bound %.3e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


def test_adjoint_identity_of_the_grouping(hip_device):
    from svnet_amd import group as Gr
    N, S, nsample, D = 300, 33, 8, 61
    x, c, pts, g, _ = _group_inputs("gauss", N, S, nsample, D, 0.3)
    idx = _group_ref("gauss", N, S, nsample, D, 0.3)[0]
    tx, tc, tp, tg, ti = _dev(hip_device, x, c, pts, g, idx)
    fwd = Gr.group_points(tx, tc, ti, tp).cpu().numpy().astype(np.float64)[..., 3:]          # the copied columns: exact
    bwd = Gr.group_points_backward(tg, ti, N).cpu().numpy().astype(np.float64)
    lhs, rhs = float((fwd * g[..., 3:]).sum()), float((pts.astype(np.float64) * bwd).sum())
    bound = sum(float((np.abs(pts[b]) * PG.group_bwd_f64(g[b], idx[b], N)[1]).sum()) for b in range(B))
    print("grouping: <fwd(f), g> %.9f, <f, bwd(g)> %.9f, difference %.3e of bound %.3e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


# ---- refusals on the device
def test_refusals_on_the_device(hip_device):
    from svnet_amd import group as Gr, propagate as Pr
    dev = hip_device
    q, r, f = _dev(dev, *R.gauss_case(65, B, 10, 5, 4))
    x, c, pts = _dev(dev, *G.gauss_case(65, B, 10, 5, 4))
    idx = torch.zeros(B, 5, 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="out="):
        Pr.propagate(q, r, f.clone().requires_grad_(), out=torch.empty(B, 4, 10, device=dev))
    with pytest.raises(ValueError, match="out="):
        Gr.group_points(x, c, idx, pts.clone().requires_grad_(), out=torch.empty(B, 5, 3, 7, device=dev))
    with pytest.raises(ValueError, match="requires grad"):
        Pr.propagate(q.clone().requires_grad_(), r, f)
    with pytest.raises(ValueError, match="requires grad"):
        Gr.group_points(x.clone().requires_grad_(), c, idx, pts)
    with pytest.raises(ValueError, match="requires grad"):
        Gr.Grouper(B, 10, 5, 3, 4, dev).run(x, c, 0.3, pts.clone().requires_grad_())
    with pytest.raises(ValueError, match="requires grad"):
        Pr.Propagator(B, 4, 5, 10, dev).run(q, r, f.clone().requires_grad_())
    # an index outside [0, N) is clamped in the backward as in the forward: the gradient lands on the clamped point
    far = torch.tensor([[[-5, 0, 99]]], dtype=torch.int64, device=dev)
    w = torch.tensor([[[0.5, 0.25, 0.125]]], device=dev)
    got = Pr.three_interpolate_backward(torch.tensor([[[2.0]]], device=dev), far, w, 3)
    assert got.flatten().tolist() == [1.5, 0.0, 0.25]


# ---- a captured graph
def test_backward_in_a_captured_graph(hip_device):
    """group_points -> max over nsample -> three_interpolate -> a fixed linear loss, forward and backward captured on a side stream
    after a warm-up; two replays with the inputs refilled in place between them each give the eager gradient bit for bit."""
    from svnet_amd import group as Gr, propagate as Pr
    dev = hip_device
    N, S, nsample, D, P = 128, 32, 8, 8, 200

    def inputs(seed):
        x, c, pts = G.gauss_case(seed, B, N, S, D, every=1)
        idx = G.query_ball_batch(x, c, G.r2_of(0.4), nsample)[0]
        q = R.gauss_case(seed, B, P, S, 1)[0]
        idx3, _, w3 = R.three_nn_batch(q, c)
        return _dev(dev, x, c, pts, idx, idx3, w3)

    sets = [inputs(80), inputs(81)]
    lw = _dev(dev, synth.normal(80, 9, (B, D, P)))[0]
    x, c, pts, idx, idx3, w3 = (t.clone() for t in sets[0])
    pts.requires_grad_()

    def gradient():
        grouped = Gr.group_points(x, c, idx, pts)                                       # [B,S,nsample,3+D]
        feat = grouped[..., 3:].max(dim=2)[0].permute(0, 2, 1).contiguous()             # [B,D,S]
        loss = (Pr.three_interpolate(feat, idx3, w3) * lw).sum()
        return torch.autograd.grad(loss, pts)[0]

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        gradient()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = gradient()
    for s in (sets[1], sets[0]):
        with torch.no_grad():
            for dst, src in zip((x, c, pts, idx, idx3, w3), s):
                dst.copy_(src)
        res.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = res.clone()
        eager = gradient()
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
        assert float(replayed.abs().max()) > 0


# ---- the modules against the reference's recorded stack
def test_module_stack_equals_the_recorded_reference(hip_device):
    from svnet_amd.models.utils import pointnet_util as U
    dev = hip_device
    mods = PG.stack_modules(U)
    for m, mod in mods.items():
        mod.load_state_dict({k[len("gc_sd:") + len(m) + 1:]: torch.from_numpy(GOLDEN[k]) for k in GOLDEN.files if k.startswith("gc_sd:%s." % m)},
                            strict=True)
        mod.to(dev).train()
    xyz, feat, lw, start = _dev(dev, GOLDEN["gc_xyz"], GOLDEN["gc_feat"], GOLDEN["gc_lw"], GOLDEN["gc_start"])
    feat.requires_grad_()
    outs = PG.stack_forward(mods, xyz, feat, lambda m, x, f: m(x, f, start=start))
    loss = (outs["out:u0"] * lw).sum()
    loss.backward()
    got = {k: v.detach().cpu().numpy() for k, v in outs.items()}
    got["out:loss"] = np.array([float(loss.detach())])
    got["dx:feat"] = feat.grad.cpu().numpy()
    for m, mod in mods.items():
        for k, p in mod.named_parameters():
            got["d:%s.%s" % (m, k)] = p.grad.cpu().numpy()
    ref = {k[3:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(("gc_out:", "gc_d:", "gc_dx:"))}
    assert set(ref) == set(got)
    assert np.array_equal(_bits(got["out:l1_xyz"]), _bits(ref["out:l1_xyz"]))            # the sampled centres: bit for bit
    worst = compare_case(got, ref, 1e-3, "SA -> SA(group_all) -> FP -> FP")
    print("module stack: worst relative error %.3e at %s" % worst)
