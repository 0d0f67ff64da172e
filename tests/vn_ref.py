"""numpy restatement of the fused vector-neuron edge level (svnet_amd/csrc/vn_edge.hip), written from the contract in
svnet_amd/vn_fused.py's docstring and include/svnet_hip.h and independent of the kernels.

    fold(w_feat, w_dir, gamma, beta, mean, var, eps)     {Af, Df [O,C], Ad, Dd [Od,C], s, t [O]} in fp32, every operation rounded once
    fold_bn(gamma, beta, mean, var, eps)                 (s, t): the ONE restatement of BatchNorm's fold, the tail's too
    fold_state(state, prefix, eps, fold=fold)            a fold from a state_dict's arrays: prefix "conv1." ...
    tables(x, f)                                         (Pn, Pc [N,O,3], Qn, Qc [N,Od,3]): the c-ascending fmaf chains from +0
    norm_leaky(p, d, s, t, slope)                        (y, dot): the ONE restatement of the norm and the leaky rule, the tail's too
    level(x, idx, f, slope, taken=None)                  [O,3,N] float32: edge, norm, leaky and mean of the contract, indices clamped
    level_batch(x, idx, f, slope)                        the same over a leading batch axis
    level_f64(x, idx, w_feat, w_dir, ...)                the module's own definition in float64 on the unfolded arrays
    synthetic_state(keys, shapes, seed)                  seeded parameters for a state_dict layout: running statistics away from their
                                                         identity start, BatchNorm weights of both signs
fmaf is tests/sa_fused_ref.fmaf: the correctly rounded fp32 fma.  numpy's float32 sum, product, quotient and square root are
correctly rounded single operations.
"""
import numpy as np

from svnet_amd import synth
from tests.sa_fused_ref import fmaf

F32, F64 = np.float32, np.float64
EPS = F32(1e-6)

# ---- the case of tests/golden/vn.npz: (seed, B, N, k, num_class), the reference's VN_DGCNN_CLS with pooling = 'mean' in eval mode
# (tests/golden/make_vn_golden.py).  Its four edge levels are the level cases: (C, O) per level.
GOLDEN_CASE = (2, 2, 64, 8, 40)
LEVEL_WIDTHS = ((1, 21), (21, 21), (21, 42), (42, 85))
LEVEL_PREFIXES = ("conv1.", "conv2.", "conv3.", "conv4.")
SLOPE = 0.2
# the small graph-feature case: (seed, B, C, N, k)
GRAPH_CASE = (5, 2, 2, 6, 3)


def fold_bn(gamma, beta, mean, var, eps):
    gamma, beta, mean, var = (np.ascontiguousarray(a, dtype=F32) for a in (gamma, beta, mean, var))
    invstd = (F32(1) / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    s = (gamma * invstd).astype(F32)
    return s, (beta - (mean * s).astype(F32)).astype(F32)


def fold(w_feat, w_dir, gamma, beta, mean, var, eps=1e-5):
    w_feat, w_dir = (np.ascontiguousarray(a, dtype=F32) for a in (w_feat, w_dir))
    C = w_feat.shape[1] // 2
    assert w_feat.shape[1] == 2 * C == w_dir.shape[1] and w_dir.shape[0] in (w_feat.shape[0], 1)
    s, t = fold_bn(gamma, beta, mean, var, eps)
    return dict(Af=np.ascontiguousarray(w_feat[:, :C]), Df=(w_feat[:, C:] - w_feat[:, :C]).astype(F32),
                Ad=np.ascontiguousarray(w_dir[:, :C]), Dd=(w_dir[:, C:] - w_dir[:, :C]).astype(F32), s=s, t=t)


def fold_state(state, prefix, eps=1e-5, fold=fold):
    return fold(state[prefix + "map_to_feat.weight"], state[prefix + "map_to_dir.weight"], state[prefix + "batchnorm.bn.weight"],
                state[prefix + "batchnorm.bn.bias"], state[prefix + "batchnorm.bn.running_mean"], state[prefix + "batchnorm.bn.running_var"], eps)


def _chain(x, M, u=None):
    """x [C,3,N], M [R,K], u [R,3] or None for +0 -> [N,R,3]: acc = u, then acc = fmaf(x[c,a,n], M[r,c], acc) for c ascending over C."""
    C, _, N = x.shape
    acc = np.zeros((N, M.shape[0], 3), dtype=F32) if u is None else np.ascontiguousarray(np.broadcast_to(u[None], (N, M.shape[0], 3)), dtype=F32)
    for c in range(C):
        acc = fmaf(x[c].T[:, None, :], M[None, :, c, None], acc)
    return acc


def tables(x, f):
    x = np.ascontiguousarray(x, dtype=F32)
    return _chain(x, f["Af"]), _chain(x, f["Df"]), _chain(x, f["Ad"]), _chain(x, f["Dd"])


def _dot3(a, b):
    return fmaf(a[..., 2], b[..., 2], fmaf(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F32)))


def norm_leaky(p, d, s, t, slope):
    """p, d [N,O,3], s, t [O] -> (y [N,O,3], dot [N,O]): the norm through BatchNorm's folded affine, then the leaky rule."""
    slope = F32(slope)
    one_minus = F32(F32(1) - slope)
    q = _dot3(p, p)
    r = (np.sqrt(q).astype(F32) + EPS).astype(F32)
    g = (fmaf(r, s[None, :], t[None, :]) / r).astype(F32)
    u = (p * g[..., None]).astype(F32)
    dot, dd = _dot3(u, d), _dot3(d, d)
    c = (dot / (dd + EPS).astype(F32)).astype(F32)
    w = np.where((dot >= 0)[..., None], u, fmaf(-c[..., None], d, u))
    return fmaf(slope, u, (one_minus * w).astype(F32)), dot


def level(x, idx, f, slope=SLOPE, taken=None):
    """x [C,3,N] float32, idx [N,k] -> [O,3,N] float32.  taken: a list that receives the share of (edge, o) pairs on the dot < 0 branch."""
    Pn, Pc, Qn, Qc = tables(x, f)
    N, k = idx.shape
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    acc = np.zeros(Pn.shape, dtype=F32)                                           # [N,O,3]
    neg = 0
    for j in range(k):
        p = (Pn[m[:, j]] + Pc).astype(F32)                                        # [N,O,3]
        d = np.broadcast_to((Qn[m[:, j]] + Qc).astype(F32), p.shape)              # (one direction row serves every o)
        y, dot = norm_leaky(p, d, f["s"], f["t"], slope)
        acc = (acc + y).astype(F32)
        neg += int((dot < 0).sum())
    if taken is not None:
        taken.append(neg / float(dot.size * k))
    out = (acc / F32(k)).astype(F32)
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def level_batch(x, idx, f, slope=SLOPE):
    return np.stack([level(x[b], idx[b], f, slope) for b in range(x.shape[0])])


def level_f64(x, idx, w_feat, w_dir, gamma, beta, mean, var, eps=1e-5, slope=SLOPE):
    """The module's definition in float64 on the unfolded arrays: [x_j - x_i | x_i] -> linear, x / (|x| + EPS) * bn(|x| + EPS), the leaky
    rule, the mean over k.  x [C,3,N], idx [N,k] -> [O,3,N] float64."""
    x, w_feat, w_dir = (np.asarray(a, dtype=F64) for a in (x, w_feat, w_dir))
    gamma, beta, mean, var = (np.asarray(a, dtype=F64) for a in (gamma, beta, mean, var))
    N = x.shape[2]
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    nb = x[:, :, m]                                                               # [C,3,N,k]
    edge = np.concatenate([nb - x[:, :, :, None], np.broadcast_to(x[:, :, :, None], nb.shape)], axis=0)
    p = np.einsum("oc,cank->oank", w_feat, edge)
    d = np.broadcast_to(np.einsum("oc,cank->oank", w_dir, edge), p.shape)
    norm = np.sqrt((p * p).sum(1)) + 1e-6
    bn = (norm - mean[:, None, None]) / np.sqrt(var + eps)[:, None, None] * gamma[:, None, None] + beta[:, None, None]
    p = p / norm[:, None] * bn[:, None]
    dot = (p * d).sum(1, keepdims=True)
    mask = (dot >= 0).astype(F64)
    y = slope * p + (1 - slope) * (mask * p + (1 - mask) * (p - dot / ((d * d).sum(1, keepdims=True) + 1e-6) * d))
    return y.mean(-1)


def synthetic_state(keys, shapes, seed):
    """{key: array} for a state_dict layout: keys and their shapes (a scalar is ()).  Linear weights ~ N(0, 1/fan_in), their biases
    ~ 0.1 N; BatchNorm weights 0.25 + N (both signs), biases 0.2 N, running means 0.25 N, running variances U(0.5, 1.5); a
    num_batches_tracked of 3.  Every draw is a function of (seed, key) alone."""
    out, keys = {}, [str(k) for k in keys]
    for key, shape in zip(keys, shapes):
        shape = tuple(int(v) for v in shape if int(v) >= 0)
        sid, leaf = synth.stream_id(key), key.rsplit(".", 1)[-1]
        norm = key[: -len(leaf)] + "running_mean" in keys
        if leaf == "num_batches_tracked":
            out[key] = np.full((), 3, dtype=np.int64)
            continue
        if leaf == "running_mean":
            a = synth.normal(seed, sid, shape) * F32(0.25)
        elif leaf == "running_var":
            a = synth.uniform(seed, sid, shape, 0.5, 1.5)
        elif leaf == "weight" and norm:
            a = synth.normal(seed, sid, shape) + F32(0.25)
        elif leaf == "bias" and norm:
            a = synth.normal(seed, sid, shape) * F32(0.2)
        elif leaf == "weight":
            a = synth.normal(seed, sid, shape) / np.sqrt(F32(shape[1]))
        elif leaf == "bias":
            a = synth.normal(seed, sid, shape) * F32(0.1)
        else:
            raise KeyError("no synthetic rule for %s" % key)
        out[key] = np.ascontiguousarray(a, dtype=F32)
    return out


def golden_cloud():
    """The golden case's input x [B,3,N]: points in the unit ball's cube, multiples of 2^-10."""
    seed, B, N, k, _ = GOLDEN_CASE
    return (np.round(synth.uniform(seed, 1, (B, 3, N), -1.0, 1.0) * 1024) / 1024).astype(F32)


def graph_inputs():
    """The small graph-feature case: x [B,C,3,N] of integers (every difference and cross product exact) and idx [B,N,k]."""
    seed, B, C, N, k = GRAPH_CASE
    x = (synth.integers(seed, 1, (B, C, 3, N), 17) - 8).astype(F32)
    return x, synth.integers(seed, 2, (B, N, k), N)
