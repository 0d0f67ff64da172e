"""numpy restatement of the fused two-layer vector-neuron edge level (svnet_amd/csrc/vn_edge2.hip) and of the per-point frame coordinates
(svnet_vn_std_coords_f32 in svnet_amd/csrc/vn_tail.hip), written from the contracts in svnet_amd/vn_fused.py (vn_edge2_mean),
svnet_amd/vn_tail.py (vn_std_coords) and include/svnet_hip.h and independent of the kernels.  Built on tests/vn_ref.py (the tables, the
norm / leaky rule, the chain) and tests/vn_tail_ref.py (the point fold, the frame rows).

    level2(x, idx, f1, f2, slope1, slope2, taken=None)   [O2,3,N] float32: layer 1 per edge as vn_ref.level has it, layer 2 as a c-ascending
                                                         fmaf chain from +0 over layer 1's outputs, the j-ascending sum, / fl(k)
    level2_batch(...)                                    the same over a leading batch axis
    level2_f64(x, idx, a1, a2, slope1, slope2)           the modules' own definition in float64 on the unfolded arrays a1, a2
    std_coords(x, y, w_lin)                              [3C,N] float32: e[3 i + k, n], the frame rows and coordinates rules of std_pool
    std_coords_f64(x, y, w_lin)                          the module's einsum in float64
    pseg_state(keys, shapes, seed)                       vn_ref.synthetic_state with the BatchNorms that the model registers twice
                                                         (bn8 and conv8.1, ...) holding one set of arrays
"""
import numpy as np

from svnet_amd import synth
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.sa_fused_ref import fmaf

F32, F64 = np.float32, np.float64
SLOPE = V.SLOPE
# ---- the case of tests/golden/vn_pseg.npz: (seed, B, N, k, num_part), the reference's VN_DGCNN_PSEG with pooling = 'mean' in eval mode
# (tests/golden/make_vn_pseg_golden.py).  The levels: the prefixes of the layers applied per edge and (C, widths...).
GOLDEN_CASE = (2, 2, 64, 8, 50)
LEVEL_PREFIXES = (("conv1.", "conv2."), ("conv3.", "conv4."), ("conv5.",))
LEVEL_WIDTHS = ((1, 21, 21), (21, 21, 21), (21, 21))
GOLDEN_LABELS = (3, 11)         # the object categories of the case's two clouds
SHARED_NORMS = ((7, "conv7"), (8, "conv8"), (9, "conv9"), (10, "conv10"))
POOLED, LABEL, COORDS = 2046, 64, 189


def golden_label():
    """l [B,16] one-hot float32: two different categories."""
    l = np.zeros((GOLDEN_CASE[1], 16), dtype=F32)
    for b, c in enumerate(GOLDEN_LABELS):
        l[b, c] = 1
    return l


def pseg_state(keys, shapes, seed):
    state = V.synthetic_state(keys, shapes, seed)
    for n, conv in SHARED_NORMS:
        for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            state["bn%d.%s" % (n, leaf)] = state["%s.1.%s" % (conv, leaf)]
    return state


def _second(y1, f2, slope2):
    """y1 [N,O1,3] -> (y2 [N,O2,3], dot [N,O2]): the chain over O1 per row of [Wf | Wd] stacked, then the norm / leaky rule."""
    W = np.concatenate([f2["Wf"], f2["Wd"]], axis=0)
    O2 = f2["Wf"].shape[0]
    assert W.shape[1] == y1.shape[1]
    acc = V._chain(np.ascontiguousarray(y1.transpose(1, 2, 0)), W)                # [N,R,3]
    p = acc[:, :O2]
    d = np.broadcast_to(acc[:, O2:], p.shape) if W.shape[0] == O2 + 1 and O2 != 1 else acc[:, O2:]
    return V.norm_leaky(p, d, f2["s"], f2["t"], slope2)


def level2(x, idx, f1, f2, slope1=SLOPE, slope2=SLOPE, taken=None):
    """x [C,3,N] float32, idx [N,k], f1 a vn_ref.fold, f2 a vn_tail_ref.fold_point -> [O2,3,N] float32.  taken: a list that receives
    (the share of (edge, channel) pairs on the dot < 0 branch in layer 1, in layer 2)."""
    Pn, Pc, Qn, Qc = V.tables(x, f1)
    N, k = idx.shape
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    acc = np.zeros((N, f2["Wf"].shape[0], 3), dtype=F32)
    neg = [0, 0]
    size = [0, 0]
    for j in range(k):
        p = (Pn[m[:, j]] + Pc).astype(F32)
        d = np.broadcast_to((Qn[m[:, j]] + Qc).astype(F32), p.shape)
        y1, dot1 = V.norm_leaky(p, d, f1["s"], f1["t"], slope1)
        y2, dot2 = _second(y1, f2, slope2)
        acc = (acc + y2).astype(F32)
        for i, dot in enumerate((dot1, dot2)):
            neg[i] += int((dot < 0).sum())
            size[i] += dot.size
    if taken is not None:
        taken.append((neg[0] / float(size[0]), neg[1] / float(size[1])))
    return np.ascontiguousarray((acc / F32(k)).astype(F32).transpose(1, 2, 0))


def level2_batch(x, idx, f1, f2, slope1=SLOPE, slope2=SLOPE):
    return np.stack([level2(x[b], idx[b], f1, f2, slope1, slope2) for b in range(x.shape[0])])


def _layer_f64(feat, a, slope):
    """feat [K,3,N,k] float64 -> [O,3,N,k]: linear, x / (|x| + EPS) * bn(|x| + EPS), the leaky rule, on the unfolded arrays a."""
    w_feat, w_dir, gamma, beta, mean, var = (np.asarray(a[key], dtype=F64) for key in ("w_feat", "w_dir", "gamma", "beta", "mean", "var"))
    p = np.einsum("oc,cank->oank", w_feat, feat)
    d = np.broadcast_to(np.einsum("oc,cank->oank", w_dir, feat), p.shape)
    norm = np.sqrt((p * p).sum(1)) + 1e-6
    bn = (norm - mean[:, None, None]) / np.sqrt(var + 1e-5)[:, None, None] * gamma[:, None, None] + beta[:, None, None]
    p = p / norm[:, None] * bn[:, None]
    dot = (p * d).sum(1, keepdims=True)
    mask = (dot >= 0).astype(F64)
    return slope * p + (1 - slope) * (mask * p + (1 - mask) * (p - dot / ((d * d).sum(1, keepdims=True) + 1e-6) * d))


def level2_f64(x, idx, a1, a2, slope1=SLOPE, slope2=SLOPE):
    """The modules' definition in float64: [x_j - x_i | x_i] -> layer 1 -> layer 2 -> the mean over k.  x [C,3,N], idx [N,k] -> [O2,3,N]."""
    x = np.asarray(x, dtype=F64)
    N = x.shape[2]
    m = np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1)
    nb = x[:, :, m]
    edge = np.concatenate([nb - x[:, :, :, None], np.broadcast_to(x[:, :, :, None], nb.shape)], axis=0)
    return _layer_f64(_layer_f64(edge, a1, slope1), a2, slope2).mean(-1)


def std_coords(x, y, w_lin):
    """x [C,3,N], y [Cy,3,N], w_lin [3,Cy] -> e [3C,N] float32, row 3 i + k."""
    x, y, w_lin = (np.ascontiguousarray(a, dtype=F32) for a in (x, y, w_lin))
    z = T.frame_rows(y, w_lin)
    vi, zk = x[:, None], z[None]                                                  # [C,1,3,N], [1,3,3,N]
    e = fmaf(vi[:, :, 2], zk[:, :, 2], fmaf(vi[:, :, 1], zk[:, :, 1], (vi[:, :, 0] * zk[:, :, 0]).astype(F32)))
    return np.ascontiguousarray(e.reshape(-1, x.shape[2]))


def std_coords_f64(x, y, w_lin):
    x, y, w_lin = (np.asarray(a, dtype=F64) for a in (x, y, w_lin))
    return np.einsum("ian,kan->ikn", x, np.einsum("kc,can->kan", w_lin, y)).reshape(-1, x.shape[2])


def golden_cloud():
    """The golden case's input x [B,3,N]: points in the unit ball's cube, multiples of 2^-10."""
    seed, B, N, k, _ = GOLDEN_CASE
    return (np.round(synth.uniform(seed, 1, (B, 3, N), -1.0, 1.0) * 1024) / 1024).astype(F32)
