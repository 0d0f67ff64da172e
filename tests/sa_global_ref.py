"""numpy restatement of the fused global set-abstraction level (svnet_amd/csrc/sa_global.hip), written from the contract in
svnet_amd/sa_global.py's docstring and include/svnet_hip.h and independent of the kernels: a few lines over tests/sa_fused_ref.py.

The global level is one group of ALL N points of a cloud, in order, around centre 0, coordinates first: sa_fused_ref's level with
new_xyz = zeros [1,3] and idx = arange(N) [1,N].  Its centred coordinates fl(x - 0) are x bit for bit (x - (+0) is exact, -0 included).

    level(xyz, points, layers)          xyz [3,N], points [D,N] or None, channel-first as the kernel takes them -> [C_out] float32
    level_f64(...)                      (value, bound) [C_out] float64: sa_fused_ref.level_f64's running bound
    *_batch                             the same over a leading batch axis -> [B,C_out,1]
"""
import numpy as np

from tests import sa_fused_ref as R

F32 = np.float32


def _group(xyz, points):
    x = np.ascontiguousarray(np.asarray(xyz, dtype=F32).T)
    pts = None if points is None else np.ascontiguousarray(np.asarray(points, dtype=F32).T)
    return x, np.zeros((1, 3), dtype=F32), np.arange(x.shape[0], dtype=np.int64)[None, :], pts


def level(xyz, points, layers):
    return R.level(*_group(xyz, points), layers)[:, 0]


def level_f64(xyz, points, layers):
    value, bound = R.level_f64(*_group(xyz, points), layers)
    return value[:, 0], bound[:, 0]


def level_batch(xyz, points, layers):
    return np.stack([level(xyz[b], None if points is None else points[b], layers) for b in range(xyz.shape[0])])[:, :, None]


def level_f64_batch(xyz, points, layers):
    per = [level_f64(xyz[b], None if points is None else points[b], layers) for b in range(xyz.shape[0])]
    return np.stack([p[0] for p in per])[:, :, None], np.stack([p[1] for p in per])[:, :, None]


# ---- the case of tests/golden/sa_global.npz: (seed, B, N, D, mlp), the reference's PointNetSetAbstraction(None, None, None, D + 3, mlp,
# True) in eval mode on lattice coordinates (tests/golden/make_sa_global_golden.py): a width past 256, N no multiple of 16.
GOLDEN_CASE = (61, 2, 40, 5, (12, 16, 260))


def golden_inputs():
    """(xyz [B,3,N] on the 2^-10 lattice in [-1, 1), points [B,D,N]) of the golden case, channel-first."""
    from svnet_amd import synth
    from tests.pointset_ref import lattice
    seed, B, N, D, _ = GOLDEN_CASE
    x = np.ascontiguousarray(lattice(seed, 1, (B, N, 3)).astype(F32).transpose(0, 2, 1))
    return x, np.ascontiguousarray(synth.normal(seed, 4, (B, N, D)).transpose(0, 2, 1))
