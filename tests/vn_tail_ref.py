"""numpy restatement of the fused vector-neuron tail (svnet_amd/csrc/vn_tail.hip), written from the contract in svnet_amd/vn_tail.py's
docstring and include/svnet_hip.h and independent of the kernels.

    fold_point(w_feat, w_dir, gamma, beta, mean, var, eps)   {Wf [O,K], Wd [Od,K], s, t [O]}: s and t are tests/vn_ref.fold_bn's
    fold_point_state(state, prefix, eps)                     the same from a state_dict's arrays: prefix "conv5." ...
    cloud_term(g, W, C)                                      [R,3]: u = +0, then fmaf over the Cg constant channels, c ascending
    point_level(x, f, slope, g=None)                         [O,3,N]: the chain from the cloud term, then tests/vn_ref.norm_leaky
    ordered_mean(e)                                          over the last axis: runs of 64 n-ascending, the runs j-ascending, / fl(N)
    std_pool(x, y, w_lin, g=None)                            [6 I]: frame rows, coordinates, [max | ordered mean]
    pooled(feats, state, slope)                              the whole tail in front of the head: the four levels' outputs -> [B, 6 I]
    *_f64                                                    the modules' own definitions in float64 on the unfolded arrays
fmaf is tests/sa_fused_ref.fmaf: the correctly rounded fp32 fma.  numpy's float32 sum, product, quotient and square root are
correctly rounded single operations.
"""
import numpy as np

from tests.sa_fused_ref import fmaf
from tests.vn_ref import SLOPE, _chain, fold_bn, fold_state, norm_leaky

F32, F64 = np.float32, np.float64
RUN = 64
# the tail of VN_DGCNN_CLS: (C, Cg, O, Od) of conv5, vn1, vn2 and (C, Cg, Cy) of the standardise-and-pool stage
MODEL_POINT = ((169, 0, 341, 1), (341, 341, 341, 341), (341, 0, 170, 170))
MODEL_STD = (341, 341, 170)
TAIL_PREFIXES = ("conv5.", "std_feature.vn1.", "std_feature.vn2.")


def fold_point(w_feat, w_dir, gamma, beta, mean, var, eps=1e-5):
    w_feat, w_dir = (np.ascontiguousarray(a, dtype=F32) for a in (w_feat, w_dir))
    assert w_feat.shape[1] == w_dir.shape[1] and w_dir.shape[0] in (w_feat.shape[0], 1)
    s, t = fold_bn(gamma, beta, mean, var, eps)
    return dict(Wf=w_feat, Wd=w_dir, s=s, t=t)


def fold_point_state(state, prefix, eps=1e-5):
    return fold_state(state, prefix, eps, fold_point)


def cloud_term(g, W, C):
    """g [Cg,3], W [R,K] with K = C + Cg -> u [R,3]."""
    u = np.zeros((W.shape[0], 3), dtype=F32)
    for c in range(g.shape[0]):
        u = fmaf(g[None, c, :], W[:, C + c, None], u)
    return u


def point_level(x, f, slope=SLOPE, g=None):
    """x [C,3,N] float32, g [Cg,3] or None -> [O,3,N] float32."""
    x = np.ascontiguousarray(x, dtype=F32)
    C = x.shape[0]
    W = np.concatenate([f["Wf"], f["Wd"]], axis=0)
    O = f["Wf"].shape[0]
    assert W.shape[1] == C + (0 if g is None else g.shape[0])
    acc = _chain(x, W, None if g is None or g.shape[0] == 0 else cloud_term(np.ascontiguousarray(g, dtype=F32), W, C))
    p, d = acc[:, :O], np.broadcast_to(acc[:, O:], (acc.shape[0], O, 3)) if W.shape[0] == O + 1 else acc[:, O:]
    return np.ascontiguousarray(norm_leaky(p, d, f["s"], f["t"], slope)[0].transpose(1, 2, 0))


def ordered_sum(e):
    """Over the last axis: run j holds n in [64 j, 64 j + 64); a run's sum is n-ascending from +0, the runs are added j-ascending from +0."""
    e = np.asarray(e, dtype=F32)
    N = e.shape[-1]
    total = np.zeros(e.shape[:-1], dtype=F32)
    for j in range(0, N, RUN):
        run = np.zeros(e.shape[:-1], dtype=F32)
        for n in range(j, min(N, j + RUN)):
            run = (run + e[..., n]).astype(F32)
        total = (total + run).astype(F32)
    return total


def ordered_mean(e):
    return (ordered_sum(e) / F32(np.asarray(e).shape[-1])).astype(F32)


def frame_rows(y, w_lin):
    """y [Cy,3,N], w_lin [3,Cy] -> z [3 k, 3 a, N]."""
    z = np.zeros((3,) + y.shape[1:], dtype=F32)
    for c in range(y.shape[0]):
        z = fmaf(y[None, c], w_lin[:, c, None, None], z)
    return z


def std_pool(x, y, w_lin, g=None):
    """x [C,3,N], y [Cy,3,N], w_lin [3,Cy], g [Cg,3] or None -> h [6 I], I = C + Cg: [max | mean] of column 3 i + k."""
    x, y, w_lin = (np.ascontiguousarray(a, dtype=F32) for a in (x, y, w_lin))
    N = x.shape[2]
    v = x if g is None or g.shape[0] == 0 else np.concatenate([x, np.broadcast_to(np.asarray(g, dtype=F32)[:, :, None], g.shape + (N,))], axis=0)
    z = frame_rows(y, w_lin)
    vi, zk = v[:, None], z[None]                                                  # [I,1,3,N], [1,3,3,N]
    e = fmaf(vi[:, :, 2], zk[:, :, 2], fmaf(vi[:, :, 1], zk[:, :, 1], (vi[:, :, 0] * zk[:, :, 0]).astype(F32)))      # [I,3,N]
    e = e.reshape(-1, N)
    return np.concatenate([e.max(axis=1), ordered_mean(e)]).astype(F32)


def pooled(feats, state, slope=SLOPE):
    """feats: the four levels' outputs [B,C_i,3,N]; state: the model's state_dict arrays -> (h [B, 6 I], the stages of cloud 0...)."""
    x = np.concatenate([np.asarray(f, dtype=F32) for f in feats], axis=1)
    f5, f1, f2 = (fold_point_state(state, p) for p in TAIL_PREFIXES)
    w_lin = np.ascontiguousarray(state["std_feature.vn_lin.weight"], dtype=F32)
    out = []
    for b in range(x.shape[0]):
        local = point_level(x[b], f5, slope)
        m = ordered_mean(local)
        y = point_level(point_level(local, f1, slope, g=m), f2, slope)
        out.append(std_pool(local, y, w_lin, g=m))
    return np.stack(out)


# ---- the modules' own definitions in float64
def point_level_f64(x, w_feat, w_dir, gamma, beta, mean, var, eps=1e-5, slope=SLOPE):
    """x [K,3,N] (constant channels expanded) -> [O,3,N] float64: linear, x / (|x| + EPS) * bn(|x| + EPS), the leaky rule."""
    x, w_feat, w_dir, gamma, beta, mean, var = (np.asarray(a, dtype=F64) for a in (x, w_feat, w_dir, gamma, beta, mean, var))
    p = np.einsum("oc,can->oan", w_feat, x)
    d = np.broadcast_to(np.einsum("oc,can->oan", w_dir, x), p.shape)
    norm = np.sqrt((p * p).sum(1)) + 1e-6
    bn = (norm - mean[:, None]) / np.sqrt(var + eps)[:, None] * gamma[:, None] + beta[:, None]
    p = p / norm[:, None] * bn[:, None]
    dot = (p * d).sum(1, keepdims=True)
    mask = (dot >= 0).astype(F64)
    return slope * p + (1 - slope) * (mask * p + (1 - mask) * (p - dot / ((d * d).sum(1, keepdims=True) + 1e-6) * d))


def std_pool_f64(x, y, w_lin):
    """x [I,3,N] (constant channels expanded), y [Cy,3,N], w_lin [3,Cy] -> [6 I] float64."""
    x, y, w_lin = (np.asarray(a, dtype=F64) for a in (x, y, w_lin))
    z = np.einsum("kc,can->kan", w_lin, y)
    e = np.einsum("ian,kan->ikn", x, z).reshape(-1, x.shape[2])
    return np.concatenate([e.max(axis=1), e.mean(axis=1)])


def expanded(x, g):
    """[x | g expanded over the points]: [C + Cg, 3, N]."""
    return np.concatenate([x, np.broadcast_to(np.asarray(g)[:, :, None], g.shape + (x.shape[2],))], axis=0)
