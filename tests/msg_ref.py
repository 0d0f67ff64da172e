"""numpy restatement of the multi-scale grouping (svnet_amd/csrc/group.hip), written from the contract in
svnet_amd/group.py's docstring ("Multi-scale grouping") and independent of the kernels.  It is built on the single-scale restatements:
tests/group_ref.py's query_ball and distances, tests/pointset_grad_ref.py's reverse lists and ordered sum.

    offsets(nsamples)                          off_i = nsample_0 + .. + nsample_(i-1)
    query_ball_msg(x, c, r2s, nsamples)        idx_cat [S,Ktot] int64, count [S,R] int32: G.query_ball per scale, laid end to end
    group_msg(x, c, idx_cat, nsamples, pts)    R arrays [S,nsample_i,D+3]: the attributes, THEN point minus centre; indices clamped
    group_msg_bwd(dgs, idx_cat, nsamples, N)   dpoints [N,D]: t_i = column c of the gradient of the scale slot j lies in, summed over
                                               the reverse lists of idx_cat in ascending edge e = s Ktot + j
    group_msg_bwd_f64                          (value, bound): the same sums in float64 and L * 2^-23 * sum|t_i| per element
    *_batch                                    the same over a leading batch axis
    scanned_fraction(idx_cat, count, nsamples, N)      per scale and for the union (the one-pass kernel scans as far as its slowest scale)
"""
import numpy as np

from svnet_amd import synth
from tests import group_ref as G
from tests import pointset_grad_ref as PG

F32 = np.float32


def offsets(nsamples):
    return [int(v) for v in np.concatenate([[0], np.cumsum(nsamples)[:-1]])]


def query_ball_msg(x, c, r2s, nsamples):
    assert len(r2s) == len(nsamples) >= 1
    per = [G.query_ball(x, c, r2, k) for r2, k in zip(r2s, nsamples)]
    return np.ascontiguousarray(np.concatenate([p[0] for p in per], axis=1)), np.ascontiguousarray(np.stack([p[1] for p in per], axis=1))


def split(idx_cat, nsamples):
    return [idx_cat[..., o:o + k] for o, k in zip(offsets(nsamples), nsamples)]


def group_msg(x, c, idx_cat, nsamples, pts=None):
    x, c = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c, dtype=F32)
    assert idx_cat.shape[1] == sum(nsamples)
    outs = []
    for idx in split(idx_cat, nsamples):
        i = np.clip(idx, 0, x.shape[0] - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            centred = (x[i] - c[:, None, :]).astype(F32)
        out = centred if pts is None else np.concatenate([np.ascontiguousarray(pts, dtype=F32)[i], centred], axis=2)
        assert out.dtype == F32
        outs.append(np.ascontiguousarray(out))
    return outs


def _terms(dgs, nsamples, dtype):
    """[D, S*Ktot]: the gradients of the scales side by side along the slot axis, the attribute columns only."""
    assert all(g.shape[1] == k for g, k in zip(dgs, nsamples))
    cat = np.concatenate([np.asarray(g, dtype=dtype) for g in dgs], axis=1)            # [S,Ktot,D+3]
    D = cat.shape[2] - 3
    assert D >= 1
    return cat.reshape(-1, cat.shape[2])[:, :D].T


def group_msg_bwd(dgs, idx_cat, nsamples, N):
    return np.ascontiguousarray(PG.ordered_sums(_terms(dgs, nsamples, F32), *PG.reverse_lists(idx_cat, N)).T)


def group_msg_bwd_f64(dgs, idx_cat, nsamples, N):
    """(sum [N,D] float64, bound [N,D]): tests/pointset_grad_ref.py's bound, L 2^-23 sum|t_i| for a list of L terms."""
    terms = _terms(dgs, nsamples, np.float64)
    rev_start, _ = PG.reverse_lists(idx_cat, N)
    target = np.clip(np.asarray(idx_cat, dtype=np.int64).reshape(-1), 0, N - 1)
    total = np.stack([np.bincount(target, weights=t, minlength=N) for t in terms])
    mag = np.stack([np.bincount(target, weights=np.abs(t), minlength=N) for t in terms])
    return total.T, (np.diff(rev_start)[None, :] * 2.0 ** -23 * mag).T


def query_ball_msg_batch(x, c, r2s, nsamples):
    return tuple(np.stack(a) for a in zip(*(query_ball_msg(x[b], c[b], r2s, nsamples) for b in range(x.shape[0]))))


def group_msg_batch(x, c, idx_cat, nsamples, pts=None):
    per = [group_msg(x[b], c[b], idx_cat[b], nsamples, None if pts is None else pts[b]) for b in range(x.shape[0])]
    return [np.stack([p[i] for p in per]) for i in range(len(nsamples))]


def group_msg_bwd_batch(dgs, idx_cat, nsamples, N):
    return np.stack([group_msg_bwd([g[b] for g in dgs], idx_cat[b], nsamples, N) for b in range(idx_cat.shape[0])])


def scanned_fraction(idx_cat, count, nsamples, N):
    """([fraction per scale], fraction of the union): G.scanned_fraction's figure per scale; the one-pass kernel leaves a centre
    when its slowest scale is full, so it scans the maximum over the scales."""
    seen = []
    for i, idx in enumerate(split(idx_cat, nsamples)):
        last = idx[..., nsamples[i] - 1]
        seen.append(np.where(count[..., i] >= nsamples[i], np.minimum((last // 64 + 1) * 64, N), N))
    return [float(s.mean()) / N for s in seen], float(np.maximum.reduce(seen).mean()) / N


# ---- the cases of tests/golden/msg.npz: name -> (seed, B, N, npoint, radii, nsamples, D, mlp_list).  Clouds of two densities - a
# core of CORE points in [-1/4, 1/4)^3 and the rest over [-1, 1)^3, all multiples of 2^-10 - so that every scale has full groups (core
# centres) and partial ones (outliers).  Radii 0.125, 0.25, 0.5 have squares exact in fp32 and, per cloud, one point planted ON each
# scale's sphere around the first centre; the squares of 0.1, 0.2, 0.4 are no multiple of 2^-20.
GOLDEN_CASES = {
    "exact": (41, 2, 256, 32, (0.125, 0.25, 0.5), (4, 8, 16), 0, ((8, 8), (8, 12), (8, 16))),
    "pp": (42, 2, 256, 32, (0.1, 0.2, 0.4), (8, 16, 32), 4, ((8, 8), (8, 12), (8, 16))),
}
CORE = 160


def planted_indices(start, R):
    """Where golden_inputs puts the on-sphere points of a cloud whose sampling starts at `start`: the R lowest indices other than it."""
    return [i for i in range(R + 1) if i != int(start)][:R]


def golden_inputs(name, start):
    """(xyz [B,N,3], points [B,N,D] or None) of a golden case, given the start indices [B] of its sampling."""
    seed, B, N, S, radii, nsamples, D, _ = GOLDEN_CASES[name]
    x = G.lattice(seed, 1, (B, N, 3))
    x[:, :CORE] = np.floor(x[:, :CORE] * 256) / 1024                   # multiples of 2^-10 in [-1/4, 1/4)
    order = np.argsort(synth.integers(seed, 2, (N,), 1 << 62), kind="stable")
    x = np.ascontiguousarray(x[:, order])                              # core points at scattered indices
    if all(r in G.EXACT_RADII for r in radii):
        for b in range(B):
            for i, r in zip(planted_indices(start[b], len(radii)), radii):
                p = x[b, int(start[b])].copy()
                p[0] = p[0] + F32(r) if p[0] + F32(r) < 1 else p[0] - F32(r)
                x[b, i] = p
    pts = synth.normal(seed, 4, (B, N, D)) if D else None
    return np.ascontiguousarray(x.astype(F32)), pts
