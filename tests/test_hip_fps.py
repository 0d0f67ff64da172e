"""GPU tests (-m gpu) of farthest point sampling and the resampled pool: svnet_fps_f32 / svnet_pool_gather_f32 (svnet_amd/csrc/fps.hip)
through svnet_amd.data against the numpy restatement tests/fps_ref.py and the reference's recorded index lists
(tests/golden/fps.npz).  Index lists are compared bit for bit; every reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fps_ref as F

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fps.npz"))
FIXED_P = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 2048, 4097, 10000, 16384]
MAX_P = 16384
_REF = {}


def _tier(P):
    from svnet_amd import _lib
    return _lib.lib().svnet_fps_tier(P)


def _tier_edges():
    """The last P of every tier but the last, and the first P of the next: computed from the query, not copied from the kernel."""
    edges, lo = [], 1
    while True:
        t = _tier(lo)
        a, b = lo, MAX_P                       # the largest P with tier(P) == t (the tier is non-decreasing in P: tests/test_host_fps.py)
        while a < b:
            mid = (a + b + 1) // 2
            a, b = (mid, b) if _tier(mid) == t else (a, mid - 1)
        if a == MAX_P:
            return edges
        edges += [a, a + 1]
        lo = a + 1


def _clouds(P, M=3):
    """Finite Gaussian clouds [M,P,3] (any P >= 1)."""
    return np.ascontiguousarray(synth.normal(4000 + P, 0, (M, P, 3)))


def _starts(P, M):
    return np.array([(0, P - 1, P // 2)[m % 3] for m in range(M)], dtype=np.int64)


def _ref(key, clouds, npoint, start):
    if key not in _REF:
        _REF[key] = F.fps_batch(clouds, npoint, start)
        _REF[key].setflags(write=False)
    return _REF[key]


def _run(dev, clouds, npoint, start):
    from svnet_amd.data import farthest_point_sample
    idx = farthest_point_sample(torch.from_numpy(clouds).to(dev), npoint, torch.from_numpy(np.asarray(start, dtype=np.int64)).to(dev))
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (clouds.shape[0], npoint)
    return idx.cpu().numpy()


def _same(got, want, tag):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d indices differ, first at %r: got %d, want %d" % (
        tag, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_every_tier_boundary_is_covered():
    edges = _tier_edges()
    tiers = sorted({_tier(P) for P in FIXED_P + edges})
    assert tiers == list(range(_tier(MAX_P) + 1)), tiers
    assert len(edges) == 2 * _tier(MAX_P) and all(_tier(a) + 1 == _tier(b) for a, b in zip(edges[::2], edges[1::2]))


def _all_p():
    try:
        return sorted(set(FIXED_P + _tier_edges()))
    except Exception:                 # the library is missing: the cases above still fail, at the import in the test
        return FIXED_P


@pytest.mark.parametrize("P", _all_p())
def test_sampler_equals_the_restatement(P, hip_device):
    """M = 3 clouds started at 0, P-1 and mid-cloud, npoint = min(P, 48)."""
    clouds, npoint, start = _clouds(P), min(P, 48), _starts(P, 3)
    _same(_run(hip_device, clouds, npoint, start), _ref(("p", P), clouds, npoint, start), "P %d (tier %d)" % (P, _tier(P)))


@pytest.mark.parametrize("P,npoint", [(65, 65), (1024, 1024), (10000, 1024)])
def test_full_length_runs(P, npoint, hip_device):
    clouds, start = _clouds(P, 2), np.array([P - 1, P // 3], dtype=np.int64)
    got = _run(hip_device, clouds, npoint, start)
    _same(got, _ref(("full", P), clouds, npoint, start), "P %d npoint %d" % (P, npoint))
    if npoint == P:
        assert all(sorted(r.tolist()) == list(range(P)) for r in got)


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_start_positions(where, hip_device):
    P = 1000
    s = {"first": 0, "last": P - 1, "middle": P // 2}[where]
    clouds, start = _clouds(P), np.full(3, s, dtype=np.int64)
    got = _run(hip_device, clouds, 48, start)
    assert (got[:, 0] == s).all()
    _same(got, _ref(("start", s), clouds, 48, start), where)


def test_heavy_ties_grid_and_repeated_points(hip_device):
    grid = F.grid_cloud()[None]
    assert grid.shape == (1, 343, 3)
    _same(_run(hip_device, grid, 100, [11]), _ref("grid", grid, 100, [11]), "7^3 grid")
    rep = F.repeated_cloud()[None]
    assert rep.shape == (1, 40, 3)
    got = _run(hip_device, rep, 16, [15])
    _same(got, _ref("rep", rep, 16, [15]), "8 points x 5")
    assert (got[0, 8:] == 0).all() and len(set(got[0, :8].tolist())) == 8       # exhausted after 8: index 0 from then on


def _padded_grid(P, positions):
    """A shuffled 4^3 integer grid (64 points, heavy ties) at `positions` of a cloud of P points; every other point is a copy of the
    grid point at positions[0], where the run starts: those copies sit at distance 0 from the first centroid and never win."""
    g = F.grid_cloud(seed=9, n=4)
    cloud = np.repeat(g[:1], P, axis=0)
    cloud[np.asarray(positions)] = g
    return np.ascontiguousarray(cloud[None]), np.array([positions[0]], dtype=np.int64)


@pytest.mark.parametrize("layout", ["lanes", "waves", "same_lane"])
@pytest.mark.parametrize("P", [256, 1024, 4096, 10240, 16384])
def test_tied_maxima_in_other_lanes_waves_and_registers(P, layout, hip_device):
    """The tied maxima of the grid sit in neighbouring lanes of one wave (points 0..63), are spread over the whole cloud (stride P/64:
    other waves and, from 1024 points on, other registers of a lane), or sit one workgroup width apart (the registers of ONE lane,
    where a lane keeps more than one point).  The first index must win every time."""
    k = np.arange(64)
    if layout == "lanes":
        pos = k
    elif layout == "waves":
        pos = k * (P // 64)
    else:
        threads = 256 if P <= 1024 else 1024           # the workgroup widths of DESIGN.md's tier table
        ppl = max(1, P // threads)
        pos = (k % ppl) * threads + k // ppl
    cloud, start = _padded_grid(P, pos.tolist())
    got = _run(hip_device, cloud, 40, start)
    want = _ref(("pad", P, layout), cloud, 40, start)
    _same(got, want, "%s P %d" % (layout, P))
    assert set(want[0].tolist()) <= set(pos.tolist())                        # (40 < 64: only grid points are ever selected)


def test_more_clouds_than_compute_units(hip_device):
    M, P = 300, 64
    clouds, start = _clouds(P, M), _starts(P, M)
    _same(_run(hip_device, clouds, 8, start), _ref("many", clouds, 8, start), "M 300")


@pytest.mark.parametrize("name", list(F.golden_cases()))
def test_golden_index_lists(name, hip_device):
    clouds, npoint = F.golden_cases()[name]
    want = GOLDEN["fps_" + name]
    _same(_run(hip_device, clouds, npoint, want[:, 0]), want, name)


def test_two_runs_are_identical(hip_device):
    clouds, start = _clouds(10000, 2), np.array([5, 9999], dtype=np.int64)
    a = _run(hip_device, clouds, 256, start)
    b = _run(hip_device, clouds, 256, start)
    assert np.array_equal(a, b)


def test_refusals(hip_device):
    from svnet_amd._lib import SvnetHipError
    from svnet_amd.data import farthest_point_sample
    x = torch.from_numpy(_clouds(100, 2))
    s = torch.zeros(2, dtype=torch.int64)
    xd, sd = x.to(hip_device), s.to(hip_device)
    with pytest.raises(RuntimeError):
        farthest_point_sample(x, 10, s)                                   # CPU tensors
    with pytest.raises(TypeError):
        farthest_point_sample(xd.double(), 10, sd)
    with pytest.raises(TypeError):
        farthest_point_sample(xd, 10, sd.int())
    with pytest.raises(ValueError):
        farthest_point_sample(xd.permute(1, 0, 2), 2, torch.zeros(100, dtype=torch.int64, device=hip_device))     # not contiguous
    with pytest.raises(ValueError):
        farthest_point_sample(xd[:, :, :2].contiguous(), 10, sd)          # not [B,P,3]
    with pytest.raises(ValueError):
        farthest_point_sample(xd, 10, sd[:1])
    with pytest.raises(SvnetHipError):
        farthest_point_sample(xd, 101, sd)                                # npoint > P
    with pytest.raises(SvnetHipError):
        farthest_point_sample(xd, 0, sd)
    with pytest.raises(SvnetHipError):
        farthest_point_sample(torch.zeros(1, 16385, 3, device=hip_device), 8, sd[:1])
    for bad in (-1, 100):
        with pytest.raises(ValueError):
            farthest_point_sample(xd, 10, torch.tensor([0, bad], dtype=torch.int64, device=hip_device))


# ---- the resampled pool
def _pool_arrays(P, M=5):
    data = _clouds(P, M).copy()
    data[M - 1] = data[M - 1] * np.float32(0.01) + np.float32(50.0)          # one cloud far from the origin
    rng_bits = synth._splitmix64(np.uint64(77 + P) * np.uint64(1 << 32) + np.arange(M * P + M, dtype=np.uint64))
    seg = (rng_bits[:M * P] % np.uint64(50)).astype(np.int64).reshape(M, P)
    label = (rng_bits[M * P:] % np.uint64(40)).astype(np.int64)
    return data, label, seg


@pytest.mark.parametrize("P,N", [(2048, 1024), (10000, 64), (64, 64)], ids=lambda v: str(v))
def test_resampled_pool(P, N, hip_device):
    from svnet_amd.data import BatchLoader, DevicePool, epoch_order, fps_start
    data, label, seg = _pool_arrays(P)
    M = data.shape[0]
    pool = DevicePool(data, label, seg, device=hip_device)
    start = fps_start(3, M, P)
    want_idx = _ref(("pool", P, N), data, N, start)
    rows = np.arange(M)[:, None]
    new = pool.resample_fps(N, seed=3)
    assert isinstance(new, DevicePool) and (new.M, new.P) == (M, N) and new.device == pool.device
    _same(new.fps_index.cpu().numpy(), want_idx, "fps_index P %d N %d" % (P, N))
    assert np.array_equal(new.data.cpu().numpy().view(np.uint32), data[rows, want_idx].view(np.uint32))
    assert np.array_equal(new.seg.cpu().numpy(), seg[rows, want_idx])
    assert new.label is pool.label and np.array_equal(new.label.cpu().numpy(), label)
    # an explicit start gives the same pool; without seg there is no seg
    again = pool.resample_fps(N, start=start)
    assert torch.equal(again.fps_index, new.fps_index) and torch.equal(again.data.view(torch.int32), new.data.view(torch.int32))
    assert DevicePool(data, label, device=hip_device).resample_fps(N, seed=3).seg is None

    normed = pool.resample_fps(N, seed=3, normalize=True)
    got = normed.data.cpu().numpy()
    assert torch.equal(normed.fps_index, new.fps_index) and torch.equal(normed.seg, new.seg)
    for m in range(M):
        sel = data[m, want_idx[m]]
        want = F.normalize_f32(sel)
        same = got[m].view(np.uint32) == want.view(np.uint32)
        assert same.all(), "cloud %d: %d of %d coordinates differ from the fp32 restatement" % (m, (~same).sum(), same.size)
        err, bound = float(abs(got[m].astype(np.float64) - F.normalize_f64(sel)).max()), F.bound_f32(sel)
        print("P %d N %d cloud %d: |fp32 - f64| %.3e, bound %.3e (%.2f of it)" % (P, N, m, err, bound, err / bound))
        assert err <= bound, (m, err, bound)
    assert torch.equal(normed.data.view(torch.int32), pool.resample_fps(N, seed=3, normalize=True).data.view(torch.int32))

    # the result is an ordinary pool: the loader takes it
    loader = BatchLoader(new, 4, N, select="first_ordered", scale_shift=False, rotate="none", seed=1)
    assert loader.load(0) == 4
    order = epoch_order(1, 0, M)[:4]
    assert torch.equal(loader.x.view(torch.int32), new.data[torch.from_numpy(order).to(hip_device)].permute(0, 2, 1).contiguous().view(torch.int32))
    assert torch.equal(loader.seg, new.seg[torch.from_numpy(order).to(hip_device)])
