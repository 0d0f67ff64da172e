"""numpy restatement of the gradients of the grouping and of the interpolation (svnet_amd/csrc/pointset_grad.hip), written from the
contract in the docstrings of svnet_amd/group.py and svnet_amd/propagate.py and independent of the kernels.

    reverse_lists(idx, N)                    idx [R,K] -> rev_start [N+1], rev_edge [R*K] int32: edge e = r K + j points to
                                             clip(idx[r,j], 0, N-1); list n holds its edges in ascending e (a STABLE argsort)
    interpolate_bwd(dout, idx, w, N)         dfeat [D,N]: per list t_i = fl(dout[d,p_i] w[p_i,j_i]), summed in list order, each
                                             addition rounded to fp32; one term gives t_1 itself, no term +0
    group_bwd(dgrouped, idx, N)              dpoints [N,D]: t_i = dgrouped[s_i,j_i,3+c], the same sum
    *_f64                                    (value, bound): the same sums in float64 and L * 2^-23 * sum|t_i| per element for a
                                             list of length L (see bound below)
    *_batch                                  the same over a leading batch axis
"""
import numpy as np

F32 = np.float32


def reverse_lists(idx, N):
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.ndim == 2 and N >= 1
    target = np.clip(idx.reshape(-1), 0, N - 1)
    rev_edge = np.argsort(target, kind="stable").astype(np.int32)                  # by target, ascending e among equals
    rev_start = np.concatenate([[0], np.cumsum(np.bincount(target, minlength=N))]).astype(np.int32)
    return rev_start, rev_edge


def ordered_sums(terms, rev_start, rev_edge):
    """terms [C,E] float32 -> [C,N] float32: column n = fl(fl(t_1 + t_2) + t_3) ... over list n in list order."""
    terms = np.ascontiguousarray(terms, dtype=F32)
    N = len(rev_start) - 1
    out = np.zeros((terms.shape[0], N), dtype=F32)                                 # an empty list: +0
    length = np.diff(rev_start)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(int(length.max()) if N else 0):                             # the i-th term of every list that has one
            has = np.flatnonzero(length > i)
            t = terms[:, rev_edge[rev_start[has] + i]]
            out[:, has] = t if i == 0 else (out[:, has] + t).astype(F32)
    assert out.dtype == F32
    return out


def _interp_terms(dout, w, dtype):
    """[D,3P]: term e = 3 p + j is dout[d,p] w[p,j]."""
    dout, w = np.asarray(dout, dtype=dtype), np.asarray(w, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return (dout[:, :, None] * w[None, :, :]).astype(dtype).reshape(dout.shape[0], -1)


def interpolate_bwd(dout, idx, w, N):
    """dout [D,P], idx [P,3], w [P,3] -> dfeat [D,N] float32."""
    return ordered_sums(_interp_terms(dout, w, F32), *reverse_lists(idx, N))


def group_bwd(dgrouped, idx, N):
    """dgrouped [S,nsample,3+D], idx [S,nsample] -> dpoints [N,D] float32."""
    dgrouped = np.ascontiguousarray(dgrouped, dtype=F32)
    terms = dgrouped.reshape(-1, dgrouped.shape[2])[:, 3:].T
    return np.ascontiguousarray(ordered_sums(terms, *reverse_lists(idx, N)).T)


def _sums_f64(terms, idx, N):
    """terms [C,E] float64 -> (sum [C,N] float64, bound [C,N]).  bound: a sum of L fp32 terms added one after the other makes L - 1
    rounding errors, each at most 2^-24 of a partial sum, itself at most sum|t_i|; the fp32 product behind a term (the
    interpolation) adds 2^-24 |t_i|: (L - 1 + 1) 2^-24 sum|t_i| <= L 2^-23 sum|t_i| with a factor two to spare for the
    second-order terms."""
    rev_start, rev_edge = reverse_lists(idx, N)
    target = np.clip(np.asarray(idx, dtype=np.int64).reshape(-1), 0, N - 1)
    total = np.zeros((terms.shape[0], N))
    mag = np.zeros((terms.shape[0], N))
    for c in range(terms.shape[0]):
        total[c] = np.bincount(target, weights=terms[c], minlength=N)
        mag[c] = np.bincount(target, weights=np.abs(terms[c]), minlength=N)
    return total, np.diff(rev_start)[None, :] * 2.0 ** -23 * mag


def interpolate_bwd_f64(dout, idx, w, N):
    return _sums_f64(_interp_terms(dout, w, np.float64), idx, N)


def group_bwd_f64(dgrouped, idx, N):
    d = np.asarray(dgrouped, dtype=np.float64)
    total, bound = _sums_f64(d.reshape(-1, d.shape[2])[:, 3:].T, idx, N)
    return total.T, bound.T


def reverse_lists_batch(idx, N):
    return tuple(np.stack(a) for a in zip(*(reverse_lists(idx[b], N) for b in range(idx.shape[0]))))


def interpolate_bwd_batch(dout, idx, w, N):
    return np.stack([interpolate_bwd(dout[b], idx[b], w[b], N) for b in range(dout.shape[0])])


def group_bwd_batch(dgrouped, idx, N):
    return np.stack([group_bwd(dgrouped[b], idx[b], N) for b in range(dgrouped.shape[0])])


# The golden stack of tests/golden/pointset_grad.npz (c): SA -> SA(group_all) -> FP -> FP of the reference's modules, train mode.
STACK = dict(seed=3, B=2, N=128, S=32, radius=0.25, nsample=8, D=4, sa1=[16, 16], sa2=[16, 16], fp2=[16], fp1=[16, 8])
# the grouping cases of (a): names of tests/group_ref.GOLDEN_CASES with D > 0
GROUP_CASES = ("r025", "r05", "r01", "r02", "r04", "big")


def stack_modules(U):
    """The four modules of the golden stack from a module namespace U (the reference's pointnet_util or svnet_amd's)."""
    c = STACK
    return {"sa1": U.PointNetSetAbstraction(c["S"], c["radius"], c["nsample"], 3 + c["D"], c["sa1"], False),
            "sa2": U.PointNetSetAbstraction(None, None, None, 3 + c["sa1"][-1], c["sa2"], True),
            "fp2": U.PointNetFeaturePropagation(c["sa1"][-1] + c["sa2"][-1], c["fp2"]),
            "fp1": U.PointNetFeaturePropagation(c["D"] + c["fp2"][-1], c["fp1"])}


def stack_forward(mods, xyz, feat, sa1_forward):
    """xyz [B,3,N], feat [B,D,N] -> {name: tensor} of the stack's outputs; sa1_forward(module, xyz, feat) runs the first level (the
    two implementations take the sampling's start differently)."""
    l1_xyz, l1 = sa1_forward(mods["sa1"], xyz, feat)
    l2_xyz, l2 = mods["sa2"](l1_xyz, l1)
    u1 = mods["fp2"](l1_xyz, l2_xyz, l1, l2)
    u0 = mods["fp1"](xyz, l1_xyz, feat, u1)
    return {"out:l1_xyz": l1_xyz, "out:l1": l1, "out:l2": l2, "out:u1": u1, "out:u0": u0}
