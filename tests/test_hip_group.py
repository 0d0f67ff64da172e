"""GPU tests (-m gpu) of the ball query and the grouping: svnet_ball_query_f32 / svnet_group_points_f32 (svnet_amd/csrc/group.hip)
through svnet_amd.group against the numpy restatement tests/group_ref.py and the reference's recorded results
(tests/golden/group.npz).  The contract is single-rounded fp32, so indices and counts are compared as integers and coordinates and
attributes as BIT PATTERNS: there is no tolerance.  Every reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from tests import group_ref as G

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group.npz"))
F32 = np.float32
_REF = {}


def _tile():
    try:
        from svnet_amd import group as Gr
        return Gr.tile()
    except Exception:                 # the library or the module is missing: the tests still fail, at the import in the test
        return 2048


T = _tile()
# (N, S, nsample, D, radius) at B = 2: every N in {1, 2, 63, 64, 65, 129, tile - 1, tile, tile + 1, 2 tile + 5}, every S in
# {1, 3, 5, 130} (partial workgroups of four waves x eight centres), every nsample in {1, 2, 16, 63, 64, 65, min(N, 128)} and every D
# in {0, 1, 5, 61, 64} (rows of 3, 4, 8, 64 and 67 columns: the float4 and the dword path) at least once.  The radii make full and
# partial groups both occur where the shape allows it.
CASES = [(1, 1, 1, 0, 0.4), (2, 3, 2, 1, 0.8), (63, 5, 63, 5, 0.9), (64, 130, 64, 61, 1.5), (65, 3, 65, 64, 0.9), (129, 5, 16, 0, 0.5),
         (T - 1, 130, 128, 1, 0.5), (T, 5, 63, 5, 0.4), (T + 1, 3, 65, 61, 0.4), (2 * T + 5, 130, 64, 64, 0.3), (129, 1, 128, 0, 1.0),
         (2 * T + 5, 5, 2, 5, 0.05)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _ref(key, x, c, pts, r2, nsample):
    """(idx, count, out) of the restatement, computed once."""
    if key not in _REF:
        idx, count = G.query_ball_batch(x, c, r2, nsample)
        out = G.group_batch(x, c, idx, pts)
        for a in (idx, count, out):
            a.setflags(write=False)
        _REF[key] = (idx, count, out)
    return _REF[key]


def _same_bits(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got, want) if got.dtype != F32 else (_bits(got), _bits(want))
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %r: got %r, want %r" % (
        tag, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _dev(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _run_all(dev, x, c, pts, radius, nsample):
    """The public calls on the device; Grouper.run must equal query_ball_point + group_points bit for bit."""
    from svnet_amd import group as Gr
    tx, tc, tp = _dev(dev, x, c, pts)
    B, N, S, D = x.shape[0], x.shape[1], c.shape[1], 0 if pts is None else pts.shape[2]
    idx, count = Gr.query_ball_point(radius, nsample, tx, tc, return_count=True)
    assert torch.equal(idx, Gr.query_ball_point(radius, nsample, tx, tc))
    out = Gr.group_points(tx, tc, idx, tp)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (B, S, nsample) and count.dtype == torch.int32 and tuple(count.shape) == (B, S)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, S, nsample, 3 + D) and out.is_contiguous()
    grouper = Gr.Grouper(B + 1, N, S, nsample, D, dev)
    both = grouper.run(tx, tc, radius, tp)
    assert both.data_ptr() == grouper.out.data_ptr() and tuple(both.shape) == tuple(out.shape)
    assert torch.equal(both.view(torch.int32), out.view(torch.int32))
    assert torch.equal(grouper.idx[:B], idx) and torch.equal(grouper.count[:B], count)
    return idx.cpu().numpy(), count.cpu().numpy(), out.cpu().numpy()


def _check_case(dev, key, x, c, pts, radius, nsample, tag):
    got = _run_all(dev, x, c, pts, radius, nsample)
    want = _ref(key, x, c, pts, G.r2_of(radius), nsample)
    for g, w, what in zip(got, want, ("idx", "count", "out")):
        _same_bits(g, w, "%s %s" % (tag, what))
    N = x.shape[1]
    assert ((got[0] >= 0) & (got[0] < N)).all() and ((got[1] >= 0) & (got[1] <= nsample)).all()
    return got


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("N,S,nsample,D,radius", CASES, ids=lambda v: str(v))
def test_kernels_equal_the_restatement(N, S, nsample, D, radius, kind, hip_device):
    make = G.lattice_case if kind == "lattice" else G.gauss_case
    x, c, pts = make(6000 + N + S, 2, N, S, D)
    idx, count, _ = _check_case(hip_device, (kind, N, S, nsample, D), x, c, pts, radius, nsample,
                                "%s B 2 N %d S %d nsample %d D %d" % (kind, N, S, nsample, D))
    copies = count[:, 0:min(len(range(0, S, 2)), N) * 2:2]
    assert (copies >= 1).all()                                            # a centre that is a point always finds itself
    print("%s N %d S %d nsample %d: %d full, %d partial, %d empty groups, scanned fraction %.3f"
          % (kind, N, S, nsample, (count == nsample).sum(), ((count > 0) & (count < nsample)).sum(), (count == 0).sum(),
             G.scanned_fraction(idx, count, nsample, N)))


def test_huge_radius_takes_the_first_points(hip_device):
    N, nsample = T + 1, 65
    x, c, pts = G.gauss_case(81, 2, N, 5, 1)
    idx, count, _ = _check_case(hip_device, "huge", x, c, pts, 1e4, nsample, "huge radius")
    assert (idx == np.arange(nsample)).all() and (count == nsample).all()


def test_radius_zero_and_duplicates_across_the_tile_boundary(hip_device):
    """Radius 0 with centres copied from points: only coincident points are inside (dist == 0 <= 0).  One point is duplicated at
    indices tile - 1 and tile - the last candidate of one LDS tile and the first of the next - and centre 0 sits on the pair."""
    N, S, nsample = T + 40, 9, 4
    x, c, pts = G.gauss_case(82, 2, N, S, 5, every=1)
    x[:, T] = x[:, T - 1]
    c[:, 0] = x[:, T - 1]
    idx, count, _ = _check_case(hip_device, "zero", x, c, pts, 0.0, nsample, "radius 0")
    assert (count >= 1).all() and (count[:, 0] == 2).all()
    assert (idx[:, 0] == [T - 1, T, T - 1, T - 1]).all()


def test_group_filling_inside_a_chunk_and_on_its_last_lane(hip_device):
    """N 200, nsample 5, centre at the origin, radius 1, every other point far away.  Cloud 0: three inside points below index 64 and
    four more between 70 and 100 - the group fills in the MIDDLE of the second 64-candidate step, where the slot computation and the
    early exit meet.  Cloud 1: the fifth inside point is index 127, the last lane of the second step; one more follows at 130."""
    N, nsample = 200, 5
    x = np.full((2, N, 3), 10.0, dtype=F32) + G.gauss_case(83, 2, N, 1, 0)[0]
    near = (G.gauss_case(84, 2, N, 1, 0)[0] * F32(0.2)).astype(F32)
    inside = ([3, 20, 63, 70, 75, 90, 99], [1, 2, 74, 84, 127, 130])
    for b in range(2):
        x[b, inside[b]] = near[b, inside[b]]
    c = np.zeros((2, 3, 3), dtype=F32)
    c[:, 1] = 50.0                                                        # a far centre between two real ones: an empty group
    idx, count, _ = _check_case(hip_device, "fill", x, c, None, 1.0, nsample, "mid-chunk fill")
    for s in (0, 2):
        assert idx[0, s].tolist() == [3, 20, 63, 70, 75] and idx[1, s].tolist() == [1, 2, 74, 84, 127]
    assert count.tolist() == [[5, 0, 5], [5, 0, 5]] and (idx[:, 1] == 0).all()
    idx, count, _ = _check_case(hip_device, "fill7", x, c, None, 1.0, 7, "partial after two chunks")
    assert idx[0, 0].tolist() == [3, 20, 63, 70, 75, 90, 99] and idx[1, 0].tolist() == [1, 2, 74, 84, 127, 130, 1]
    assert count.tolist() == [[7, 0, 7], [6, 0, 6]]


def test_empty_groups_and_non_finite_coordinates(hip_device):
    N, S, nsample = T + 9, 6, 8
    x, c, pts = G.gauss_case(85, 2, N, S, 1)
    c[:, 1] = [30.0, -30.0, 30.0]                                         # far from every point
    plain = _check_case(hip_device, "finite", x, c, pts, 0.4, nsample, "far centres")
    assert (plain[1][:, 1] == 0).all() and (plain[0][:, 1] == 0).all() and (plain[1][:, 0] >= 1).all()
    want_rows = np.concatenate([x[:, 0] - c[:, 1], pts[:, 0]], axis=1)    # grouped from point 0
    assert np.array_equal(_bits(plain[2][:, 1]), _bits(np.repeat(want_rows[:, None, :], nsample, axis=1)))
    x2, c2 = x.copy(), c.copy()
    c2[0, 2] = np.nan                                                     # one NaN centre
    x2[1, 5, 1] = np.inf                                                  # one infinite point
    x2[0, T + 3, 0] = -np.inf
    from svnet_amd import group as Gr
    tx, tc, tp = _dev(hip_device, x2, c2, pts)
    idx, count = Gr.query_ball_point(0.4, nsample, tx, tc, return_count=True)
    out = Gr.group_points(tx, tc, idx, tp).cpu().numpy()
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    assert ((idx >= 0) & (idx < N)).all(), (idx.min(), idx.max())
    assert count[0, 2] == 0 and (idx[0, 2] == 0).all() and np.isnan(out[0, 2, :, :3]).all()
    want_idx, want_count = G.query_ball_batch(x2, c2, G.r2_of(0.4), nsample)
    _same_bits(idx, want_idx, "non-finite idx")
    _same_bits(count, want_count, "non-finite count")
    assert not (idx[1] == 5).any() and not (idx[0] == T + 3).any()        # an infinite point is in nobody's group
    keep = np.ones((2, S), dtype=bool)
    keep[0, 2] = False
    _same_bits(out[keep], G.group_batch(x2, c2, want_idx, pts)[keep], "the other centres' rows")
    _same_bits(out[1], plain[2][1], "cloud 1 is unaffected by its infinite point")


def test_group_points_clamps_an_index_out_of_range(hip_device):
    from svnet_amd import group as Gr
    for D in (0, 1, 2):                                                   # 3 columns, the float4 path, 5 columns
        x, c, pts = G.gauss_case(86, 2, 11, 3, D)
        idx = np.tile(np.array([4, -5, 11 + 3, 10, 0], dtype=np.int64), (2, 3, 1))
        tx, tc, tp, ti = _dev(hip_device, x, c, pts, idx)
        out = Gr.group_points(tx, tc, ti, tp).cpu().numpy()
        _same_bits(out, G.group_batch(x, c, np.tile(np.array([4, 0, 10, 10, 0]), (2, 3, 1)), pts), "clamped D %d" % D)
        buf = torch.zeros(2, 3, 5, 3 + D, device=hip_device)
        assert Gr.group_points(tx, tc, ti, tp, out=buf) is buf and np.array_equal(_bits(buf.cpu().numpy()), _bits(out))
        if D == 1:                                                        # a buffer that is NOT 16-byte aligned takes the dword path
            flat = torch.zeros(2 * 3 * 5 * 4 + 1, device=hip_device)
            odd = flat[1:].view(2, 3, 5, 4)
            assert odd.data_ptr() % 16 == 4 and Gr.group_points(tx, tc, ti, tp, out=odd) is odd
            assert np.array_equal(_bits(odd.cpu().numpy()), _bits(out)) and float(flat[0]) == 0


def _sample_and_group_parts(dev, x, pts, start, S, radius, nsample):
    from svnet_amd import group as Gr
    from svnet_amd.data import farthest_point_sample
    tx, tp, ts = _dev(dev, x, pts, start)
    res = Gr.sample_and_group(S, radius, nsample, tx, tp, returnfps=True, start=ts)
    short = Gr.sample_and_group(S, radius, nsample, tx, tp, start=ts)
    assert len(res) == 4 and len(short) == 2
    assert torch.equal(short[0].view(torch.int32), res[0].view(torch.int32)) and torch.equal(short[1].view(torch.int32), res[1].view(torch.int32))
    fps = farthest_point_sample(tx, S, ts)
    centres = torch.gather(tx, 1, fps.unsqueeze(2).expand(-1, -1, 3)).contiguous()
    idx = Gr.query_ball_point(radius, nsample, tx, centres)
    grouped = Gr.group_points(tx, centres, idx, tp)
    assert torch.equal(res[3], fps) and torch.equal(res[0].view(torch.int32), centres.view(torch.int32))
    assert torch.equal(res[1].view(torch.int32), grouped.view(torch.int32))
    B = x.shape[0]
    raw = torch.stack([tx[b][idx[b]] for b in range(B)])
    assert torch.equal(res[2].view(torch.int32), raw.view(torch.int32))
    return tuple(t.cpu().numpy() for t in res) + (idx.cpu().numpy(),)


@pytest.mark.parametrize("name", list(G.GOLDEN_CASES))
def test_golden_through_the_kernels(name, hip_device):
    """sample_and_group equals farthest_point_sample + gather + query_ball_point + group_points bit for bit, and the reference's
    recorded tuple."""
    seed, B, N, S, nsample, D, radius = G.GOLDEN_CASES[name]
    x, start = GOLDEN[name + "_xyz"], GOLDEN[name + "_start"]
    pts = GOLDEN[name + "_points"] if D else None
    new_xyz, new_points, grouped_xyz, fps, idx = _sample_and_group_parts(hip_device, x, pts, start, S, radius, nsample)
    _same_bits(fps, GOLDEN[name + "_fps"], "%s fps_idx" % name)
    _same_bits(new_xyz, GOLDEN[name + "_new_xyz"], "%s new_xyz" % name)
    _same_bits(idx, GOLDEN[name + "_idx"], "%s idx" % name)
    _same_bits(new_points, GOLDEN[name + "_new_points"], "%s new_points" % name)
    _same_bits(grouped_xyz, GOLDEN[name + "_grouped_xyz"], "%s grouped_xyz" % name)


def test_sample_and_group_default_start_and_group_all(hip_device):
    from svnet_amd import group as Gr
    from svnet_amd.data import fps_start
    x, _, pts = G.gauss_case(87, 2, 150, 1, 3)
    tx, tp = _dev(hip_device, x, pts)
    a = Gr.sample_and_group(20, 0.5, 8, tx, tp, returnfps=True, seed=5)
    b = Gr.sample_and_group(20, 0.5, 8, tx, tp, returnfps=True, start=fps_start(5, 2, 150))
    assert (a[3][:, 0].cpu().numpy() == fps_start(5, 2, 150)).all()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    none = Gr.sample_and_group(20, 0.5, 8, tx, None, seed=5)
    assert tuple(none[1].shape) == (2, 20, 8, 3) and torch.equal(none[1].view(torch.int32), a[1][..., :3].contiguous().view(torch.int32))
    new_xyz, new_points = Gr.sample_and_group_all(tx, tp)
    assert tuple(new_xyz.shape) == (2, 1, 3) and float(new_xyz.abs().max()) == 0
    assert torch.equal(new_points, torch.cat([tx.view(2, 1, 150, 3), tp.view(2, 1, 150, 3)], dim=-1))
    assert torch.equal(Gr.sample_and_group_all(tx, None)[1], tx.view(2, 1, 150, 3))


def test_sample_and_group_in_a_captured_graph(hip_device):
    """sample_and_group on fixed input buffers captured on a side stream after a warm-up; two replays with the inputs refilled in
    place between them each equal the eager result on those inputs bit for bit."""
    from svnet_amd import group as Gr
    dev = hip_device
    B, N, S, nsample, D = 2, 700, 40, 16, 5
    sets = [G.gauss_case(90 + i, B, N, 1, D) for i in range(2)]
    starts = [np.array([3, 650], dtype=np.int64), np.array([699, 0], dtype=np.int64)]
    tx, tp, ts = _dev(dev, sets[0][0], sets[0][2], starts[0])
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        Gr.sample_and_group(S, 0.4, nsample, tx, tp, returnfps=True, start=ts)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = Gr.sample_and_group(S, 0.4, nsample, tx, tp, returnfps=True, start=ts)
    for (x, _, pts), start in ((sets[1], starts[1]), (sets[0], starts[0])):
        tx.copy_(torch.from_numpy(x)); tp.copy_(torch.from_numpy(pts)); ts.copy_(torch.from_numpy(start))
        for r in res:
            r.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = [r.clone() for r in res]
        eager = Gr.sample_and_group(S, 0.4, nsample, tx, tp, returnfps=True, start=ts)
        for r, e in zip(replayed, eager):
            assert r.dtype == e.dtype and torch.equal(r if r.dtype == torch.int64 else r.view(torch.int32),
                                                      e if e.dtype == torch.int64 else e.view(torch.int32))
        assert float(replayed[1].abs().max()) > 0 and (replayed[3][:, 0].cpu().numpy() == start).all()


def test_refusals_on_the_device(hip_device):
    from svnet_amd import group as Gr
    from svnet_amd._lib import SvnetHipError
    dev = hip_device
    x, c, pts = _dev(dev, *G.gauss_case(88, 2, 10, 5, 4))
    idx = torch.zeros(2, 5, 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        Gr.query_ball_point(0.2, 3, x, c.cpu())                            # mismatched devices
    with pytest.raises(SvnetHipError):
        Gr.query_ball_point(0.2, 11, x, c)                                 # nsample > N: the reference returns N columns, we refuse
    with pytest.raises(SvnetHipError):
        Gr.query_ball_point(0.2, 0, x, c)
    with pytest.raises(SvnetHipError):
        Gr.query_ball_point(0.2, 1, torch.zeros(2, 32769, 3, device=dev), c)
    with pytest.raises(SvnetHipError):
        Gr.query_ball_point(0.2, 1, x, torch.zeros(2, 0, 3, device=dev))
    with pytest.raises(SvnetHipError):
        Gr.sample_and_group(11, 0.2, 3, x, pts)                            # npoint > N
    with pytest.raises(SvnetHipError):
        Gr.Grouper(2, 10, 5, 11, 4, dev)
    with pytest.raises(ValueError):
        Gr.group_points(x, c, idx, pts, out=torch.empty(2, 5, 3, 8, device=dev))
    with pytest.raises(TypeError):
        Gr.group_points(x, c, idx, pts, out=torch.empty(2, 5, 3, 7, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        Gr.Grouper(2, 10, 5, 3, 4, dev).run(x, c, 0.2)                     # built for D = 4, run without attributes
    with pytest.raises(ValueError):
        Gr.sample_and_group(5, 0.2, 3, x, pts, start=torch.zeros(3, dtype=torch.int64, device=dev))
