"""numpy restatement of the feature propagation (svnet_amd/csrc/propagate.hip), written from the contract in svnet_amd/propagate.py's
docstring and independent of the kernels; plus the procedural inputs of the tests.

    three_nn(q, r)                 idx [P,3] int64, dist3 [P,3], weight [P,3]: every operation a single-rounded fp32 operation (numpy
                                   float32 arrays round each operation once and never fuse), a STABLE argsort for the tie rule
    three_interpolate(f, idx, w)   out [D,P] in the contract's order
    propagate(q, r, f)             the two in sequence; *_batch: the same over a leading batch axis
    interpolate_f64(q, r, f, idx)  the same function of the SAME neighbours in float64 throughout, and bound_f32: what the fp32
                                   sequence may differ from it by
"""
import numpy as np

from svnet_amd import synth
from tests.pointset_ref import distances, lattice         # noqa: F401  (the tests reach them through this module)

F32 = np.float32
EPS = F32(1e-8)
CHUNK = 512                    # query points per distance block (memory only: no effect on any result)


def weights(dist3):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rec = (F32(1.0) / (dist3 + EPS).astype(F32)).astype(F32)
        s = ((rec[:, 0] + rec[:, 1]).astype(F32) + rec[:, 2]).astype(F32)
        return (rec / s[:, None]).astype(F32)


def three_nn(q, r):
    """q [P,3], r [N,3] float32 (finite) -> idx [P,3] int64, dist3 [P,3] float32, weight [P,3] float32."""
    q, r = np.ascontiguousarray(q, dtype=F32), np.ascontiguousarray(r, dtype=F32)
    P, N = q.shape[0], r.shape[0]
    assert q.shape == (P, 3) and r.shape == (N, 3) and P >= 1 and N >= 1
    K = min(3, N)
    idx = np.zeros((P, 3), dtype=np.int64)                    # slots past K: index 0, distance +inf (hence weight 0)
    dist3 = np.full((P, 3), np.inf, dtype=F32)
    for a in range(0, P, CHUNK):
        dist = distances(q[a:a + CHUNK], r)
        order = np.argsort(dist, axis=1, kind="stable")[:, :K]          # stable: the lower index first among equals
        idx[a:a + CHUNK, :K] = order
        dist3[a:a + CHUNK, :K] = np.take_along_axis(dist, order, axis=1)
    w = weights(dist3)
    assert dist3.dtype == F32 and w.dtype == F32
    return idx, dist3, w


def three_interpolate(f, idx, w):
    """f [D,N], idx [P,3], w [P,3] -> out [D,P] float32."""
    f = np.ascontiguousarray(f, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = (f[:, idx[:, 0]] * w[None, :, 0]).astype(F32)
        t1 = (f[:, idx[:, 1]] * w[None, :, 1]).astype(F32)
        t2 = (f[:, idx[:, 2]] * w[None, :, 2]).astype(F32)
        out = ((t0 + t1).astype(F32) + t2).astype(F32)
    assert out.dtype == F32
    return out


def propagate(q, r, f):
    idx, _, w = three_nn(q, r)
    return three_interpolate(f, idx, w)


def three_nn_batch(q, r):
    return tuple(np.stack(x) for x in zip(*(three_nn(q[b], r[b]) for b in range(q.shape[0]))))


def propagate_batch(q, r, f):
    return np.stack([propagate(q[b], r[b], f[b]) for b in range(q.shape[0])])


def interpolate_f64(q, r, f, idx):
    """The contract's function of the neighbours `idx` [P,3] in float64 (slots past min(3, N) take no part)."""
    q, r, f = (np.asarray(x, dtype=np.float64) for x in (q, r, f))
    K = min(3, r.shape[0])
    d = q[:, None, :] - r[idx[:, :K]]                                   # [P,K,3]
    rec = 1.0 / ((d * d).sum(axis=2) + float(EPS))
    w = rec / rec.sum(axis=1, keepdims=True)
    return (f[:, idx[:, :K]] * w[None]).sum(axis=2)


def bound_f32(f):
    """|fp32 contract - interpolate_f64| <= 20 * 2^-24 * max|f| per output, for the same neighbours.  With u = 2^-24: each d_c carries
    u (relative), its square 3 u, the two additions of non-negative terms one u each: dist within 5 u; + 1e-8 and the reciprocal: rec
    within 7 u (fp32(1e-8) itself differs from 1e-8 by less than u); s, two additions of positive terms: 9 u; w = rec / s: 17 u.  The
    products f w and the two additions add 3 u of at most sum_j |f_j| w_j <= max|f| (the weights are positive and sum to 1 within 3 u):
    20 u max|f|, second-order terms well inside the slack of the roundings counted twice."""
    return 20.0 * 2.0 ** -24 * float(np.abs(np.asarray(f, dtype=np.float64)).max())


# ---- procedural inputs (lattice: tests/pointset_ref.py)
def lattice_case(seed, B, P, N, D):
    """(q [B,P,3], r [B,N,3], f [B,D,N]): lattice queries; every second sampled point (as far as there are queries: each is copied
    at most once) is a copy of a query, the coincident points a resampled pool consists of; Gaussian features."""
    q = lattice(seed, 1, (B, P, 3))
    r = lattice(seed, 2, (B, N, 3))
    n = min((N + 1) // 2, P)
    for b in range(B):
        pick = np.argsort(synth.integers(seed, 3 + 16 * b, (P,), 1 << 62), kind="stable")[:n]       # n DISTINCT queries
        r[b, 0:2 * n:2] = q[b, pick]
    f = synth.normal(seed, 4, (B, D, N))
    return np.ascontiguousarray(q), np.ascontiguousarray(r), np.ascontiguousarray(f)


def gauss_case(seed, B, P, N, D):
    """Seeded Gaussian clouds: the queries' first min(P, N) // 2 points reappear among the sampled points (coincident points at
    coordinates whose squares are NOT exact)."""
    q = synth.normal(seed, 1, (B, P, 3))
    r = synth.normal(seed, 2, (B, N, 3))
    n = min(P, N) // 2
    r[:, :n] = q[:, :n]
    f = synth.normal(seed, 4, (B, D, N))
    return np.ascontiguousarray(q), np.ascontiguousarray(r), np.ascontiguousarray(f)


# The cases of tests/golden/propagate.npz: name -> (seed, B, P, N, D).  Inputs are rebuilt by lattice_case; the file holds them too
# ("<name>_q", "_r", "_f"), with the reference's output "<name>_out" [B,D,P] and, for N >= 3, its neighbours "<name>_idx" [B,P,3].
GOLDEN_CASES = {
    "n37": (11, 2, 200, 37, 5),
    "n3": (12, 2, 300, 3, 4),
    "n2049": (13, 1, 64, 2049, 3),
    "n1": (14, 2, 50, 1, 4),
    "n130": (15, 1, 1000, 130, 7),
}


def distinct_smallest(q, r, count=4):
    """True when every query's `count` (or N, if fewer) smallest distances are pairwise distinct: the reference's unstable sort then
    has one possible answer."""
    for b in range(q.shape[0]):
        d = np.sort(distances(q[b], r[b]), axis=1)[:, :count]
        if d.shape[1] > 1 and (np.diff(d, axis=1) == 0).any():
            return False
    return True
