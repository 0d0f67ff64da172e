"""numpy restatement of the ball query and the grouping (svnet_amd/csrc/group.hip), written from the contract in svnet_amd/group.py's
docstring and independent of the kernels; plus the procedural inputs of the tests.

    distances(c, x)                    dist [S,N] float32 in the contract's order (tests/pointset_ref.py)
    r2_of(radius)                      fp32(radius * radius), the square taken in double
    query_ball(x, c, r2, nsample)      idx [S,nsample] int64, count [S] int32: a plain loop over the centres
    group(x, c, idx, pts)              [S,nsample,3+D]: point minus centre, then the attributes; an index outside [0, N) is clamped
    *_batch                            the same over a leading batch axis
"""
import numpy as np

from svnet_amd import synth
from tests.pointset_ref import distances, lattice         # noqa: F401  (the tests reach them through this module)

F32 = np.float32


def r2_of(radius):
    with np.errstate(over="ignore"):
        return F32(float(radius) * float(radius))


def query_ball(x, c, r2, nsample):
    """x [N,3], c [S,3] -> idx [S,nsample] int64, count [S] int32."""
    x, c = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c, dtype=F32)
    N, S = x.shape[0], c.shape[0]
    assert x.shape == (N, 3) and c.shape == (S, 3) and 1 <= nsample <= N and S >= 1
    r2 = F32(r2)
    idx = np.zeros((S, nsample), dtype=np.int64)                  # an empty group: every slot 0
    count = np.zeros((S,), dtype=np.int32)
    for s in range(S):
        with np.errstate(invalid="ignore"):
            inside = distances(c[s:s + 1], x)[0] <= r2            # a NaN distance compares false
        ids = np.flatnonzero(inside)[:nsample]                    # ascending point index
        count[s] = len(ids)
        if len(ids):
            idx[s, :len(ids)] = ids
            idx[s, len(ids):] = ids[0]
    return idx, count


def group(x, c, idx, pts=None):
    """x [N,3], c [S,3], idx [S,nsample], pts [N,D] or None -> [S,nsample,3+D] float32."""
    x, c = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c, dtype=F32)
    i = np.clip(idx, 0, x.shape[0] - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (x[i] - c[:, None, :]).astype(F32)
    if pts is not None:
        out = np.concatenate([out, np.ascontiguousarray(pts, dtype=F32)[i]], axis=2)
    assert out.dtype == F32
    return np.ascontiguousarray(out)


def query_ball_batch(x, c, r2, nsample):
    return tuple(np.stack(a) for a in zip(*(query_ball(x[b], c[b], r2, nsample) for b in range(x.shape[0]))))


def group_batch(x, c, idx, pts=None):
    return np.stack([group(x[b], c[b], idx[b], None if pts is None else pts[b]) for b in range(x.shape[0])])


def scanned_fraction(idx, count, nsample, N):
    """Mean fraction of a cloud's N points a wave of the kernel looks at before it leaves: a full group ends with the 64-candidate
    step that holds its last index, any other group takes all N (tools/time_group.py reports the same figure from device results)."""
    last = idx[..., nsample - 1]
    seen = np.where(count >= nsample, np.minimum((last // 64 + 1) * 64, N), N)
    return float(seen.mean()) / N


# ---- procedural inputs (lattice: tests/pointset_ref.py)
def _copy_centres(seed, x, c, every):
    """Centres 0, every, 2 every, ... become copies of distinct points (as far as there are points)."""
    B, N, S = x.shape[0], x.shape[1], c.shape[1]
    n = min(len(range(0, S, every)), N)
    for b in range(B):
        pick = np.argsort(synth.integers(seed, 3 + 16 * b, (N,), 1 << 62), kind="stable")[:n]      # n DISTINCT points
        c[b, 0:n * every:every] = x[b, pick]


def lattice_case(seed, B, N, S, D, every=2):
    """(xyz [B,N,3], new_xyz [B,S,3], points [B,N,D] or None): lattice points and centres; every `every`-th centre (half of them by
    default, all with every=1) is a copy of a point, what sampled centres are; Gaussian attributes."""
    x = lattice(seed, 1, (B, N, 3))
    c = lattice(seed, 2, (B, S, 3))
    _copy_centres(seed, x, c, every)
    pts = synth.normal(seed, 4, (B, N, D)) if D else None
    return np.ascontiguousarray(x), np.ascontiguousarray(c), pts


def gauss_case(seed, B, N, S, D, every=2):
    """Seeded Gaussian clouds scaled by 1/2 (coordinates whose squares are NOT exact), every `every`-th centre a copy of a point."""
    x = (synth.normal(seed, 1, (B, N, 3)) * F32(0.5)).astype(F32)
    c = (synth.normal(seed, 2, (B, S, 3)) * F32(0.5)).astype(F32)
    _copy_centres(seed, x, c, every)
    pts = synth.normal(seed, 4, (B, N, D)) if D else None
    return np.ascontiguousarray(x), np.ascontiguousarray(c), pts


# The cases of tests/golden/group.npz: name -> (seed, B, N, npoint, nsample, D, radius).  The reference's sample_and_group(npoint,
# radius, nsample, xyz, points, returnfps=True) under torch.manual_seed(seed) and its query_ball_point on the centres that gave; the
# file holds "<name>_xyz" [B,N,3], "<name>_points" [B,N,D] (D > 0), "<name>_start" [B] (the start torch.randint drew), and the results
# "<name>_fps" [B,S], "<name>_new_xyz" [B,S,3], "<name>_idx" [B,S,nsample], "<name>_new_points" [B,S,nsample,3+D],
# "<name>_grouped_xyz" [B,S,nsample,3].  Radii 0.125, 0.25, 0.5 have squares exact in fp32 and a point planted ON the sphere of the
# first centre (golden_inputs); the squares of 0.1, 0.2, 0.4 are no multiple of 2^-20.
GOLDEN_CASES = {
    "r0125": (21, 2, 300, 40, 16, 0, 0.125),
    "r025": (22, 2, 300, 40, 16, 3, 0.25),
    "r05": (23, 2, 600, 64, 16, 2, 0.5),
    "r01": (24, 2, 600, 50, 8, 1, 0.1),
    "r02": (25, 2, 300, 40, 16, 5, 0.2),
    "r04": (26, 2, 300, 40, 16, 4, 0.4),
    "big": (27, 1, 2048, 128, 32, 3, 0.4),
}
GOLDEN_SUFFIXES = ("_xyz", "_points", "_start", "_fps", "_new_xyz", "_idx", "_new_points", "_grouped_xyz")
EXACT_RADII = (0.125, 0.25, 0.5)


def planted_index(start):
    """Where golden_inputs puts the on-sphere point of a cloud whose sampling starts at `start`: a low index, so that it is among
    the first nsample inside points of the start's group."""
    return 0 if int(start) != 0 else 1


def golden_inputs(name, start):
    """(xyz, points or None) of a golden case, given the start indices [B] of its sampling.  For a radius whose square is exact the
    point at planted_index(start[b]) is moved to start's point + (radius, 0, 0) (or - radius, whichever stays inside [-1, 1)): at
    distance exactly r2 from the first centre of cloud b, which must count as inside."""
    seed, B, N, S, nsample, D, radius = GOLDEN_CASES[name]
    x = lattice(seed, 1, (B, N, 3))
    if radius in EXACT_RADII:
        for b in range(B):
            centre = x[b, int(start[b])].copy()
            centre[0] = centre[0] + F32(radius) if centre[0] + F32(radius) < 1 else centre[0] - F32(radius)
            x[b, planted_index(start[b])] = centre
    pts = synth.normal(seed, 4, (B, N, D)) if D else None
    return np.ascontiguousarray(x), pts
