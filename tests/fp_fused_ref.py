"""numpy restatement of the fused feature-propagation level (svnet_amd/csrc/fp_fused.hip), written from the contract in
svnet_amd/fp_fused.py's docstring and include/svnet_hip.h and independent of the kernels.  For one cloud (fl() is rounding to fp32,
every operation rounded once):

    input row   of point p: h0 = [ points1[0..D1-1, p] | y[0..D2-1] ], the order of cat([points1, interpolated]); points1 bit for bit,
                y[d] = fl(fl(fl(f[d,i0] w0) + fl(f[d,i1] w1)) + fl(f[d,i2] w2)), f = points2 [D2,S], w_j = weight[p,j],
                i_j = idx[p,j] clamped into 0 .. S-1; with S < 3 the empty slots are index 0 with weight 0 (three_nn writes them so).
    layers      per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc if acc > 0 else +0.
    output      out[o, p] = hL_p[o], channel-first.

    rows(idx, w, f2, f1)                       [N,D1+D2] float32: the input rows (tests/propagate_ref.three_interpolate's arithmetic)
    level(idx, w, f2, f1, layers)              [C_out,N] float32: the chain of the contract (tests/sa_fused_ref: exact fmaf, mlp)
    level_f64(...)                             (value, bound) [C_out,N] float64: the same layers in float64 on the same fp32 rows and
                                               folded weights, and tests/sa_fused_ref.py's running bound on what the fp32 chain may
                                               differ by (its docstring; the bound's n + 2 holds for n <= 1536 just as well: the
                                               second-order terms are n^2 2^-48 against n 2^-24)
    *_batch                                    the same over a leading batch axis
three_nn is tests/propagate_ref.three_nn; the fold tests/sa_fused_ref.fold; results are compared through positive_zero.
"""
import numpy as np

from tests import propagate_ref as P
from tests.sa_fused_ref import fold, fold_state, fmaf, mlp, mlp_f64, positive_zero, single_prefixes        # noqa: F401  (the tests reach them here)

F32 = np.float32


def rows(idx, w, f2, f1=None):
    """idx [N,3], w [N,3], f2 [D2,S], f1 [D1,N] or None -> [N,D1+D2] float32."""
    f2 = np.ascontiguousarray(f2, dtype=F32)
    i = np.clip(np.asarray(idx, dtype=np.int64), 0, f2.shape[1] - 1)
    y = P.three_interpolate(f2, i, np.ascontiguousarray(w, dtype=F32)).T
    if f1 is None:
        return np.ascontiguousarray(y)
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(f1, dtype=F32).T, y], axis=1))


def level(idx, w, f2, f1, layers):
    return np.ascontiguousarray(mlp(rows(idx, w, f2, f1), layers).T)


def level_f64(idx, w, f2, f1, layers):
    h, bound = mlp_f64(rows(idx, w, f2, f1), layers)
    return np.ascontiguousarray(h.T), np.ascontiguousarray(bound.T)


def level_batch(idx, w, f2, f1, layers):
    return np.stack([level(idx[b], w[b], f2[b], None if f1 is None else f1[b], layers) for b in range(f2.shape[0])])


# ---- the cases of tests/golden/fp_fused.npz: name -> (seed, B, N, S, D1, D2, widths), the reference's PointNetFeaturePropagation in
# eval mode on lattice coordinates (tests/golden/make_fp_fused_golden.py).  "s1" is the reference's `S == 1` branch, points1 = None.
GOLDEN_CASES = {
    "a": (61, 2, 96, 24, 5, 7, (12, 16)),
    "s1": (62, 2, 16, 1, 0, 6, (8,)),
}


def golden_inputs(name, seed=None):
    """(xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,D1,N] or None, points2 [B,D2,S]) of a golden case: lattice coordinates (multiples of
    2^-10), every second sampled point a copy of a dense one, Gaussian features."""
    from svnet_amd import synth
    s, B, N, S, D1, D2, _ = GOLDEN_CASES[name]
    seed = s if seed is None else seed
    q, r, f2 = P.lattice_case(seed, B, N, S, D2)
    f1 = np.ascontiguousarray(synth.normal(seed, 5, (B, D1, N))) if D1 else None
    return q, r, f1, f2


def golden_restatement(G, name):
    """The restatement's output [B,C,N] on a golden case's recorded inputs and state_dict: three_nn, then the chain."""
    _, B, N, S, D1, D2, widths = GOLDEN_CASES[name]
    state = {str(k): G["%s_sd:%s" % (name, k)] for k in G[name + "_keys"]}
    layers = fold_state(state, single_prefixes(len(widths)))
    idx, _, w = P.three_nn_batch(G[name + "_xyz1"], G[name + "_xyz2"])
    return level_batch(idx, w, G[name + "_points2"], G[name + "_points1"] if D1 else None, layers)
