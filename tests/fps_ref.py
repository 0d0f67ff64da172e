"""numpy restatement of farthest point sampling and of the resampled pool's normalisation (svnet_amd/csrc/fps.hip), written from the
semantics in svnet_amd/data.py's docstring and independent of the kernels; plus the procedural inputs the golden file does not store.

    fps(xyz, npoint, start)        the index list, every operation a single-rounded fp32 operation, the first index winning a tie
    normalize_f32(sel)             the kernel's normalisation restated bit for bit (fixed-order float64 mean rounded once to fp32)
    normalize_f64(sel)             the same function in float64 throughout (what the bounds of the tests are taken against)
"""
import numpy as np

from svnet_amd import synth

F32 = np.float32
GATHER_THREADS = 256          # the summation order of the centroid: 256 running sums, 4 butterflies of 64, then ((w0 + w1) + w2) + w3


def fps(xyz, npoint, start):
    """xyz [P,3] float32 -> [npoint] int64."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    P = xyz.shape[0]
    assert xyz.shape == (P, 3) and 1 <= npoint <= P and 0 <= start < P
    mind = np.full(P, 1e10, dtype=F32)
    idx = np.empty(npoint, dtype=np.int64)
    f = int(start)
    x, y, z = (np.ascontiguousarray(xyz[:, c]) for c in range(3))
    for i in range(npoint):
        idx[i] = f
        d0, d1, d2 = x - x[f], y - y[f], z - z[f]
        dist = (d0 * d0 + d1 * d1) + d2 * d2              # float32 arrays: numpy rounds every operation once, and never fuses
        assert dist.dtype == F32
        mind = np.where(dist < mind, dist, mind)
        f = int(np.argmax(mind))                          # numpy's argmax returns the first of equal maxima
    return idx


def fps_batch(xyz, npoint, start):
    return np.stack([fps(xyz[m], npoint, int(start[m])) for m in range(xyz.shape[0])])


def centroid_f32(sel):
    """The float64 mean of sel [N,3] float32 in the kernel's fixed order, rounded once to fp32."""
    sel = np.ascontiguousarray(sel, dtype=F32)
    N, T = sel.shape[0], GATHER_THREADS
    rows = -(-N // T)
    padded = np.zeros((rows * T, 3), dtype=np.float64)
    padded[:N] = sel
    s = np.zeros((T, 3), dtype=np.float64)
    for r in range(rows):                                 # thread t adds its points t, t + 256, .. in ascending order
        s = s + padded[r * T:(r + 1) * T]
    s = s.reshape(T // 64, 64, 3)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):                      # the xor butterfly of a wave: every lane ends with the same sum
        s = s + s[:, lanes ^ off]
    w = s[:, 0]
    total = ((w[0] + w[1]) + w[2]) + w[3]
    return (total / np.float64(N)).astype(F32)


def normalize_f32(sel):
    sel = np.ascontiguousarray(sel, dtype=F32)
    c = centroid_f32(sel)
    d = sel - c
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    m = np.sqrt(r2).max()
    assert d.dtype == F32 and m.dtype == F32
    with np.errstate(invalid="ignore", divide="ignore"):
        return d / m


def normalize_f64(sel):
    sel = np.asarray(sel, dtype=np.float64)
    d = sel - sel.mean(axis=0)
    return d / np.sqrt((d * d).sum(axis=1)).max()


def _scale(sel):
    sel = np.asarray(sel, dtype=np.float64)
    c = sel.mean(axis=0)
    return c, np.sqrt(((sel - c) ** 2).sum(axis=1)).max()


def bound_numpy_f32(sel):
    """2^-24 (8 + 2 N ||p||inf / m): |numpy float32 pc_normalize - float64| per coordinate of the unit-scale output.  numpy's float32
    mean along axis 0 is a sequential fp32 sum: up to N roundings of partial sums <= N ||p||inf, i.e. a centroid error of up to
    2^-24 N ||p||inf, which enters d and (through m) every coordinate: the factor 2.  8 covers the subtraction, the three-term norm
    with its root, and the division.  Loose on purpose: it pins "the same function"."""
    sel = np.asarray(sel, dtype=np.float64)
    _, m = _scale(sel)
    return 2.0 ** -24 * (8.0 + 2.0 * sel.shape[0] * abs(sel).max() / m)


def bound_f32(sel):
    """2^-24 (8 + 4 ||c||inf / m): |the kernel's fp32 sequence - float64|.  The centroid is the exact mean rounded once (half an ulp
    of ||c||inf) and the subtraction p - c rounds at the magnitude of its operands (another ulp of ~||c||inf for an offset cloud), each
    entering d and m: 4 ||c||inf / m in units of 2^-24; 8 as above."""
    c, m = _scale(sel)
    return 2.0 ** -24 * (8.0 + 4.0 * abs(c).max() / m)


# ---- procedural inputs (not stored in tests/golden/fps.npz)
def synth_clouds(seed, M, P):
    """The clouds of synth.cloud_batch, point-major [M,P,3]."""
    return np.ascontiguousarray(synth.cloud_batch(seed, 0, 0, M, P).transpose(0, 2, 1))


def _perm(seed, n):
    """A fixed permutation of 0..n-1 (splitmix64 keys: the same on every numpy)."""
    return np.argsort(synth._splitmix64(np.uint64(seed) * np.uint64(1 << 32) + np.arange(n, dtype=np.uint64)), kind="stable")


def grid_cloud(seed=5, n=7):
    """A shuffled n x n x n integer grid [n^3,3]: every distance is a small integer, so the maxima tie heavily."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    return np.ascontiguousarray(g[_perm(seed, g.shape[0])])


def repeated_cloud(seed=6, distinct=8, times=5):
    """`distinct` points each repeated `times` times, shuffled: past `distinct` samples every mind is 0 and index 0 is returned."""
    pts = synth_clouds(seed, 1, distinct)[0]
    return np.ascontiguousarray(np.repeat(pts, times, axis=0)[_perm(seed, distinct * times)])


def offset_cloud(seed, P, offset, scale):
    """A synthetic cloud scaled and moved away from the origin in fp32: offset +- a few scale."""
    return np.ascontiguousarray(synth_clouds(seed, 1, P)[0] * F32(scale) + F32(offset))


# The cases of tests/golden/fps.npz: name -> (clouds [M,P,3], npoint).  The file holds, per name, the reference's index lists
# "fps_<name>" [M,npoint] (column 0 = the start torch.randint drew); inputs are rebuilt here.
def golden_cases():
    return {
        "gauss1000": (synth_clouds(31, 3, 1000), 128),
        "modelnet_v2": (synth_clouds(32, 2, 10000), 1024),
        "grid343": (grid_cloud()[None], 100),
        "repeated40": (repeated_cloud()[None], 16),
        "full65": (synth_clouds(33, 2, 65), 65),
        "offset100": (offset_cloud(34, 500, 100.0, 0.01)[None], 64),
        "single": (np.array([[[0.5, -1.0, 2.0]], [[3.0, 4.0, 5.0]]], dtype=F32), 1),
    }


# pc_normalize cases: name -> selection [N,3] (N <= 128); the file holds the reference's float32 output "norm_<name>"
def norm_cases():
    c = synth_clouds(36, 1, 1000)[0]
    sel = c[fps(c, 128, 17)]
    return {
        "centred128": sel,
        "offset3": np.ascontiguousarray(sel[:100] + F32(3.0)),
        "offset50_small": offset_cloud(37, 64, 50.0, 0.01),
        "seven": np.ascontiguousarray(c[:7]),
    }
