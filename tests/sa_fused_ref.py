"""numpy restatement of the fused set-abstraction level (svnet_amd/csrc/sa_fused.hip), written from the contract in
svnet_amd/sa_fused.py's docstring and include/svnet_hip.h and independent of the kernels.

    fold(W, b, gamma, beta, mean, var, eps)          (Wf [O,C], bf [O]) in fp32, every operation rounded once
    fmaf(a, b, c)                                    fl(a b + c) with ONE rounding, on float32 arrays
    rows(x, c, idx, pts, xyz_last)                   [S,K,3+D]: the centred coordinates and the attributes, indices clamped
    level(x, c, idx, pts, layers, xyz_last)          [C_out,S] float32: the chain of the contract, then the max over a group
    mlp_f64(h, layers), level_f64(...)               (value, bound) [C_out,S] float64: the same layers in float64 on the same fp32 rows
                                                     and folded weights, and a running bound on what the fp32 chain may differ by
    *_batch                                          the same over a leading batch axis

fmaf: the product of two fp32 numbers is exact in float64 (48 bits); the sum of it and c is rounded TO ODD in float64 (the float64
sum, its exact error by TwoSum, and where the sum was inexact and came out even its odd neighbour on the error's side) and then to
fp32.  Rounding to odd at 53 bits keeps what the final rounding to 24 bits has to know - 53 >= 2 * 24 + 2 - so the result is the
correctly rounded fp32 fma; plain float64 arithmetic rounds twice and is wrong on the ties tests/test_host_sa_fused.py constructs.

The bound: a chain of n fmaf that starts at the bias is a sum of n + 1 terms, each carrying at most n + 1 roundings, so it differs from
the exact sum of its own inputs by at most (n + 2) 2^-24 (|bf| + sum |h_c| |Wf[o,c]|) (the +2 absorbs the second-order terms for
n <= 324); the inputs themselves differ by the previous layer's bound, which enters through sum |Wf[o,c]| bound_c.  ReLU and the
maximum are 1-Lipschitz: they pass a bound on, the maximum as the largest of its rows' bounds.
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS24 = 2.0 ** -24


def fold(W, b, gamma, beta, mean, var, eps):
    W, b, gamma, beta, mean, var = (np.ascontiguousarray(a, dtype=F32) for a in (W, b, gamma, beta, mean, var))
    W = W.reshape(W.shape[0], -1)
    invstd = (F32(1) / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    s = (gamma * invstd).astype(F32)
    Wf = (W * s[:, None]).astype(F32)
    bf = (((b - mean).astype(F32) * s).astype(F32) + beta).astype(F32)
    assert Wf.dtype == F32 and bf.dtype == F32
    return np.ascontiguousarray(Wf), np.ascontiguousarray(bf)


def fold_state(state, prefixes, eps=1e-5):
    """state: {key: array}; prefixes: [(conv prefix, bn prefix)] per layer, e.g. ("mlp_convs.0.", "mlp_bns.0.") -> [(Wf, bf)]."""
    return [fold(state[c + "weight"], state[c + "bias"], state[n + "weight"], state[n + "bias"], state[n + "running_mean"],
                 state[n + "running_var"], eps) for c, n in prefixes]


def fmaf(a, b, c):
    """fl(a * b + c) with one rounding, elementwise on float32 arrays (broadcast); finite operands."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    p = a.astype(F64) * b.astype(F64)                               # exact
    c = np.broadcast_to(c.astype(F64), np.broadcast(p, c).shape)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                                      # TwoSum: s + e = p + c exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def rows(x, c, idx, pts=None, xyz_last=False):
    x, c = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c, dtype=F32)
    i = np.clip(np.asarray(idx, dtype=np.int64), 0, x.shape[0] - 1)
    centred = (x[i] - c[:, None, :]).astype(F32)
    if pts is None:
        return np.ascontiguousarray(centred)
    attrs = np.ascontiguousarray(pts, dtype=F32)[i]
    return np.ascontiguousarray(np.concatenate([attrs, centred] if xyz_last else [centred, attrs], axis=2))


def mlp(h, layers):
    """h [..., C0] float32 -> [..., CL] float32: per layer acc = bf, then fmaf over c ascending, then acc > 0 ? acc : +0."""
    h = np.ascontiguousarray(h, dtype=F32)
    for Wf, bf in layers:
        assert Wf.dtype == F32 and bf.dtype == F32 and Wf.shape == (bf.shape[0], h.shape[-1])
        acc = np.broadcast_to(bf, h.shape[:-1] + bf.shape).astype(F32)
        for ch in range(h.shape[-1]):
            acc = fmaf(h[..., ch:ch + 1], Wf[:, ch], acc)
        h = np.where(acc > 0, acc, F32(0)).astype(F32)
    return h


def level(x, c, idx, pts, layers, xyz_last=False):
    """x [N,3], c [S,3], idx [S,K], pts [N,D] or None, layers [(Wf, bf)] -> [C_out,S] float32."""
    return np.ascontiguousarray(mlp(rows(x, c, idx, pts, xyz_last), layers).max(axis=1).T)


def mlp_f64(h, layers):
    """h [..., C0] float32 -> (value, bound) [..., CL] float64: the layers in float64 and the running bound (module docstring)."""
    h = h.astype(F64)
    bound = np.zeros_like(h)
    for Wf, bf in layers:
        W, b0, n = Wf.astype(F64), bf.astype(F64), Wf.shape[1]
        z = h @ W.T + b0
        mag = (np.abs(h) + bound) @ np.abs(W).T + np.abs(b0)
        bound = bound @ np.abs(W).T + (n + 2) * EPS24 * mag
        h = np.maximum(z, 0.0)
    return h, bound


def level_f64(x, c, idx, pts, layers, xyz_last=False):
    """(value, bound) [C_out,S] float64 (module docstring)."""
    h, bound = mlp_f64(rows(x, c, idx, pts, xyz_last), layers)
    return np.ascontiguousarray(h.max(axis=1).T), np.ascontiguousarray(bound.max(axis=1).T)


def level_batch(x, c, idx, pts, layers, xyz_last=False):
    return np.stack([level(x[b], c[b], idx[b], None if pts is None else pts[b], layers, xyz_last) for b in range(x.shape[0])])


def level_f64_batch(x, c, idx, pts, layers, xyz_last=False):
    per = [level_f64(x[b], c[b], idx[b], None if pts is None else pts[b], layers, xyz_last) for b in range(x.shape[0])]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])


def positive_zero(a):
    """The bit patterns of a float32 array with -0 counted as +0: what the results are compared as."""
    bits = np.ascontiguousarray(a, dtype=F32).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    return bits


# ---- the case of tests/golden/sa_fused.npz: (seed, B, N, npoint, radius, nsample, D, mlp), the reference's single-scale
# PointNetSetAbstraction in eval mode on lattice coordinates (tests/golden/make_sa_fused_golden.py).
GOLDEN_CASE = (51, 2, 256, 32, 0.25, 16, 4, (8, 12, 16))


def single_prefixes(L):
    return [("mlp_convs.%d." % i, "mlp_bns.%d." % i) for i in range(L)]


def msg_prefixes(scale, L):
    return [("conv_blocks.%d.%d." % (scale, i), "bn_blocks.%d.%d." % (scale, i)) for i in range(L)]


CORE = 160


def golden_inputs():
    """(xyz [B,N,3], points [B,N,D]) of the golden case: clouds of two densities as in tests/msg_ref.py - CORE points in
    [-1/4, 1/4)^3 and the rest over [-1, 1)^3, all multiples of 2^-10, at scattered indices - so that there are full groups (core
    centres) and padded ones (outliers)."""
    from svnet_amd import synth
    from tests.pointset_ref import lattice
    seed, B, N, S, radius, nsample, D, _ = GOLDEN_CASE
    x = lattice(seed, 1, (B, N, 3))
    x[:, :CORE] = np.floor(x[:, :CORE] * 256) / 1024
    order = np.argsort(synth.integers(seed, 2, (N,), 1 << 62), kind="stable")
    x = np.ascontiguousarray(x[:, order].astype(F32))
    return x, synth.normal(seed, 4, (B, N, D))
