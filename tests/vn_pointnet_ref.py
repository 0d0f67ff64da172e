"""numpy restatement of the fused vector-neuron position level (svnet_amd/csrc/vn_cross.hip) and of the norm-only point layer
(svnet_vn_point_norm_f32 in svnet_amd/csrc/vn_tail.hip), written from the contracts in svnet_amd/vn_pointnet.py's and
svnet_amd/vn_tail.py's docstrings and include/svnet_hip.h and independent of the kernels.

    fold_cross(w_feat, w_dir, gamma, beta, mean, var, eps)   {Wf [O,3], Wd [Od,3], s, t [O]}: s and t are tests/vn_ref.fold_bn's
    edge_feature(xi, xj)                                     [3 c, ..., 3 a]: x_j - x_i, x_i, x_j x x_i, every operation rounded once
    cross_level(x, idx, f, slope, taken=None)                [O,3,N]: edge, product, tests/vn_ref.norm_leaky and the mean, indices clamped
    cross_level_batch(x, idx, f, slope)                      the same over a leading batch axis, x [B,1,3,N]
    cross_level_f64(x, idx, arrays, slope)                   the module's own definition in float64 on the unfolded arrays
    fold_norm(w_feat, gamma, beta, mean, var, eps)           {Wf [O,C], s, t [O]}
    point_norm(x, f)                                         [O,3,N]: tests/vn_tail_ref's chain from +0, then the norm rule alone
    point_norm_f64(x, arrays)                                linear, x / (|x| + EPS) * bn(|x| + EPS) in float64
    encoder(x, idx, state)                                   the chained encoder of VN_PointNet_CLS on a folded state: its stages
fmaf is tests/sa_fused_ref.fmaf: the correctly rounded fp32 fma.  numpy's float32 sum, product, quotient and square root are
correctly rounded single operations.
"""
import numpy as np

from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.sa_fused_ref import fmaf

F32, F64 = np.float32, np.float64
EPS = V.EPS

# ---- the case of tests/golden/vn_pointnet.npz: (seed, B, N, k, num_class), the reference's VN_PointNet_CLS with pooling = 'mean' in eval
# mode (tests/golden/make_vn_pointnet_golden.py)
GOLDEN_CASE = (3, 2, 64, 8, 40)
SLOPE = 0.0                                       # every leaky rule of the model
POS_WIDTH, MID_WIDTH, WIDE, POOLED = 21, 42, 341, 2046
STAGES = ("pos", "conv1", "fstn", "conv2", "h", "logits")


def fold_cross(w_feat, w_dir, gamma, beta, mean, var, eps=1e-5):
    w_feat, w_dir = (np.ascontiguousarray(a, dtype=F32) for a in (w_feat, w_dir))
    assert w_feat.shape[1] == 3 == w_dir.shape[1] and w_dir.shape[0] in (w_feat.shape[0], 1)
    s, t = V.fold_bn(gamma, beta, mean, var, eps)
    return dict(Wf=w_feat, Wd=w_dir, s=s, t=t)


def edge_feature(xi, xj):
    """xi, xj [..., 3] float32 -> [3, ..., 3]: the three vectors of an edge, channel first."""
    def cross(a, b):
        return ((xj[..., a] * xi[..., b]).astype(F32) - (xj[..., b] * xi[..., a]).astype(F32)).astype(F32)
    return np.stack([(xj - xi).astype(F32), np.broadcast_to(xi, xj.shape).astype(F32), np.stack([cross(1, 2), cross(2, 0), cross(0, 1)], axis=-1)])


def _rows(e, W):
    """e [3 c, N, 3 a], W [R, 3] -> [N, R, 3]: acc = +0, then acc = fmaf(e_c[a], W[r,c], acc) for c = 0, 1, 2."""
    acc = np.zeros((e.shape[1], W.shape[0], 3), dtype=F32)
    for c in range(3):
        acc = fmaf(e[c][:, None, :], W[None, :, c, None], acc)
    return acc


def cross_level(x, idx, f, slope=SLOPE, taken=None):
    """x [3,N] (or [1,3,N]) float32, idx [N,k] -> [O,3,N] float32.  taken: a list that receives the share of (edge, o) pairs on the
    dot < 0 branch."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(3, -1)
    N, k = idx.shape
    assert x.shape[1] == N
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    xi = np.ascontiguousarray(x.T)                                                # [N,3]
    O = f["Wf"].shape[0]
    acc = np.zeros((N, O, 3), dtype=F32)
    neg = 0
    for j in range(k):
        e = edge_feature(xi, xi[m[:, j]])
        p = _rows(e, f["Wf"])
        d = np.broadcast_to(_rows(e, f["Wd"]), p.shape)                           # (one direction row serves every o)
        y, dot = V.norm_leaky(p, d, f["s"], f["t"], slope)
        acc = (acc + y).astype(F32)
        neg += int((dot < 0).sum())
    if taken is not None:
        taken.append(neg / float(N * O * k))
    return np.ascontiguousarray((acc / F32(k)).astype(F32).transpose(1, 2, 0))


def cross_level_batch(x, idx, f, slope=SLOPE):
    return np.stack([cross_level(x[b], idx[b], f, slope) for b in range(x.shape[0])])


def _bn_leaky_f64(p, d, a, slope):
    """p [O,3,...], d broadcastable to it -> the module's VNBatchNorm and leaky rule in float64."""
    gamma, beta, mean, var = (np.asarray(a[key], dtype=F64).reshape((-1,) + (1,) * (p.ndim - 2)) for key in ("gamma", "beta", "mean", "var"))
    norm = np.sqrt((p * p).sum(1)) + 1e-6
    p = p / norm[:, None] * ((norm - mean) / np.sqrt(var + 1e-5) * gamma + beta)[:, None]
    if d is None:
        return p
    dot = (p * d).sum(1, keepdims=True)
    mask = (dot >= 0).astype(F64)
    return slope * p + (1 - slope) * (mask * p + (1 - mask) * (p - dot / ((d * d).sum(1, keepdims=True) + 1e-6) * d))


def cross_level_f64(x, idx, a, slope=SLOPE):
    """The module's definition in float64 on the unfolded arrays a (w_feat, w_dir, gamma, beta, mean, var): x [3,N], idx [N,k] ->
    [O,3,N] float64."""
    x = np.asarray(x, dtype=F64).reshape(3, -1)
    N = x.shape[1]
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    nb = x[:, m]                                                                  # [3,N,k]
    ctr = np.broadcast_to(x[:, :, None], nb.shape)
    edge = np.stack([nb - ctr, ctr, np.cross(nb, ctr, axis=0)])                   # [3 c, 3 a, N, k]
    p = np.einsum("oc,cank->oank", np.asarray(a["w_feat"], dtype=F64), edge)
    d = np.broadcast_to(np.einsum("oc,cank->oank", np.asarray(a["w_dir"], dtype=F64), edge), p.shape)
    return _bn_leaky_f64(p, d, a, slope).mean(-1)


def fold_norm(w_feat, gamma, beta, mean, var, eps=1e-5):
    s, t = V.fold_bn(gamma, beta, mean, var, eps)
    return dict(Wf=np.ascontiguousarray(w_feat, dtype=F32), s=s, t=t)


def point_norm(x, f):
    """x [C,3,N] float32 -> [O,3,N] float32: p by the point term's chain from +0, q = fl(p0 p0) then fmaf in p1 and p2,
    r = fl(fl(sqrt(q)) + EPS), g = fl(fmaf(r, s, t) / r), out = fl(p g)."""
    p = T._chain(np.ascontiguousarray(x, dtype=F32), f["Wf"])                     # [N,O,3]
    r = (np.sqrt(V._dot3(p, p)).astype(F32) + EPS).astype(F32)
    g = (fmaf(r, f["s"][None, :], f["t"][None, :]) / r).astype(F32)
    return np.ascontiguousarray((p * g[..., None]).astype(F32).transpose(1, 2, 0))


def point_norm_f64(x, a):
    """x [C,3,N], a (w_feat, gamma, beta, mean, var) -> [O,3,N] float64."""
    return _bn_leaky_f64(np.einsum("oc,can->oan", np.asarray(a["w_feat"], dtype=F64), np.asarray(x, dtype=F64)), None, a, 0.0)


def _norm_state(state, linear, bn):
    return fold_norm(state[linear + "map_to_feat.weight"], state[bn + "bn.weight"], state[bn + "bn.bias"], state[bn + "bn.running_mean"],
                     state[bn + "bn.running_var"])


def encoder(x, idx, state, prefix="feat."):
    """x [B,3,N], idx [B,N,k], state: the model's state_dict arrays -> {stage: array} for "pos", "conv1", "fstn", "conv2", "local", "h":
    the fused path of svnet_amd.vn_pointnet.FusedVNPointNet, every layer by its restatement (the transform net's fc layers, which the
    wrapper runs in torch, as point layers on one point)."""
    fp = {key: T.fold_point_state(state, prefix + key + ".") for key in ("conv1", "conv2", "std_feature.vn1", "std_feature.vn2", "fstn.conv1",
                                                                         "fstn.conv2", "fstn.conv3", "fstn.fc1", "fstn.fc2")}
    fx = V.fold_state(state, prefix + "conv_pos.", fold=fold_cross)
    fn = _norm_state(state, prefix + "conv3.", prefix + "bn3.")
    w_fc3 = np.ascontiguousarray(state[prefix + "fstn.fc3.map_to_feat.weight"], dtype=F32)
    w_lin = np.ascontiguousarray(state[prefix + "std_feature.vn_lin.weight"], dtype=F32)
    out = {key: [] for key in ("pos", "conv1", "fstn", "conv2", "local", "h")}
    for b in range(x.shape[0]):
        pos = cross_level(x[b], idx[b], fx, SLOPE)
        x1 = T.point_level(pos, fp["conv1"], SLOPE)
        t = x1
        for key in ("fstn.conv1", "fstn.conv2", "fstn.conv3"):
            t = T.point_level(t, fp[key], SLOPE)
        g = T.ordered_mean(t)[:, :, None]                                         # [341,3,1]: one point
        for key in ("fstn.fc1", "fstn.fc2"):
            g = T.point_level(g, fp[key], SLOPE)
        g = np.ascontiguousarray(T._chain(g, w_fc3)[0])                           # [21,3]
        x2 = T.point_level(x1, fp["conv2"], SLOPE, g=g)
        local = point_norm(x2, fn)
        m = T.ordered_mean(local)
        y = T.point_level(T.point_level(local, fp["std_feature.vn1"], SLOPE, g=m), fp["std_feature.vn2"], SLOPE)
        h = T.std_pool(local, y, w_lin, g=m)[:POOLED]
        for key, v in (("pos", pos), ("conv1", x1), ("fstn", g), ("conv2", x2), ("local", local), ("h", h)):
            out[key].append(v)
    return {key: np.stack(v) for key, v in out.items()}


def head_f64(h, state, eps=1e-5):
    """h [B,2046] -> logits [B,num_class] in float64: fc1 / bn1 / relu, fc2 / bn2 / relu (dropout is the identity in eval mode), fc3."""
    h = np.asarray(h, dtype=F64)
    for i in (1, 2):
        w, b = (np.asarray(state["fc%d.%s" % (i, n)], dtype=F64) for n in ("weight", "bias"))
        gamma, beta, mean, var = (np.asarray(state["bn%d.%s" % (i, n)], dtype=F64) for n in ("weight", "bias", "running_mean", "running_var"))
        h = np.maximum(((h @ w.T + b) - mean) / np.sqrt(var + eps) * gamma + beta, 0.0)
    return h @ np.asarray(state["fc3.weight"], dtype=F64).T + np.asarray(state["fc3.bias"], dtype=F64)


def golden_cloud():
    """The golden case's input x [B,3,N]: points in the unit cube, multiples of 2^-10."""
    from svnet_amd import synth
    seed, B, N, k, _ = GOLDEN_CASE
    return (np.round(synth.uniform(seed, 1, (B, 3, N), -1.0, 1.0) * 1024) / 1024).astype(F32)


def degenerate_cloud(N=12):
    """x [1,3,N] and idx [1,N,k]: point 0 at the origin, point 2 a duplicate of point 1, and lists in which every point meets the
    origin, the duplicate pair and itself (difference and cross product exactly zero)."""
    from svnet_amd import synth
    x = synth.normal(77, 1, (1, 3, N))
    x[0, :, 0] = 0
    x[0, :, 2] = x[0, :, 1]
    idx = np.stack([np.arange(N), np.zeros(N, np.int64), np.ones(N, np.int64), np.full(N, 2), (np.arange(N) + 1) % N], axis=1)[None].astype(np.int64)
    return np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(idx)
