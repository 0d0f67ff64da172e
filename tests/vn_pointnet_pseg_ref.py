"""numpy restatement of the fused forward of VN_PointNet_PSEG (svnet_amd/vn_pointnet_pseg.py), chained from the restatements the
kernels already have - tests/vn_pointnet_ref.py (the position level, the norm-only point layer), tests/vn_tail_ref.py (the point
level, the ordered mean, the standardise-and-pool stage) and tests/vn_pseg_ref.py (the per-point coordinates) - and stating none of
them again.  The wide envelope changes no rule, so nothing here knows of it.

    encoder(x, idx, state)      {stage: [B,...] float32}: "pos", "out1" .. "out4", "fstn", "local" [682,3,N], "m" [682,3], "y" [170,3,N]
                                (vn2's output, what the frame is made of), "h" [4092] (the amax half), "trans" [3 a, 3 k, N] (the
                                frame as the module returns it), "e1234" [825,N], "e5" [2046,N] (the coordinates of local)
    head_f64(st, l, state)      the head in float64 on [h | l | e1234 | e5 | the mean's coordinates] -> logits [B,num_part,N]
"""
import numpy as np

from tests import vn_pointnet_ref as PN
from tests import vn_pseg_ref as PS
from tests import vn_ref as V
from tests import vn_tail_ref as T

F32, F64 = np.float32, np.float64
# ---- the case of tests/golden/vn_pointnet_pseg.npz: (seed, B, N, k, num_part), the reference's VN_PointNet_PSEG with pooling = 'mean'
# in eval mode (tests/golden/make_vn_pointnet_pseg_golden.py)
GOLDEN_CASE = (4, 2, 64, 8, 50)
GOLDEN_LABELS = (5, 12)         # the object categories of the case's two clouds
SLOPE = 0.0                     # every leaky rule of the model
POS_WIDTH, MID_WIDTH, LOCAL_WIDTH, WIDE = 21, 42, 170, 682
POOLED, LABEL, SKIP = 4092, 16, 825
# the strides at which the two largest recordings are kept (the fixture stays under 512 KB): out4 over its channels, e1234 over the points
OUT4_STRIDE, E1234_STRIDE = 4, 4
STAGES = ("pos", "out1", "out2", "out3", "out4", "fstn", "h", "trans", "e1234", "logits")
POINT_LAYERS = ("conv1", "conv2", "conv3", "conv4", "std_feature.vn1", "std_feature.vn2", "fstn.conv1", "fstn.conv2", "fstn.conv3", "fstn.fc1", "fstn.fc2")


def golden_cloud():
    """The golden case's input x [B,3,N]: points in the unit cube, multiples of 2^-10."""
    from svnet_amd import synth
    seed, B, N, k, _ = GOLDEN_CASE
    return (np.round(synth.uniform(seed, 1, (B, 3, N), -1.0, 1.0) * 1024) / 1024).astype(F32)


def golden_label():
    """l [B,16] one-hot float32: two different categories."""
    l = np.zeros((GOLDEN_CASE[1], LABEL), dtype=F32)
    for b, c in enumerate(GOLDEN_LABELS):
        l[b, c] = 1
    return l


def recorded(key, a):
    """A stage as the fixture keeps it: out4 and e1234 at their strides, the rest whole."""
    return a[:, ::OUT4_STRIDE] if key == "out4" else a[:, :, ::E1234_STRIDE] if key == "e1234" else a


def encoder(x, idx, state):
    """x [B,3,N], idx [B,N,k], state: the model's state_dict arrays -> {stage: array}: the fused path of
    svnet_amd.vn_pointnet_pseg.FusedVNPointNetPSeg in front of the head, every layer by its restatement (the transform net's fc
    layers, which the wrapper runs in torch, as point layers on one point)."""
    fp = {key: T.fold_point_state(state, key + ".") for key in POINT_LAYERS}
    fx = V.fold_state(state, "conv_pos.", fold=PN.fold_cross)
    fn = PN._norm_state(state, "conv5.", "bn5.")
    w_fc3 = np.ascontiguousarray(state["fstn.fc3.map_to_feat.weight"], dtype=F32)
    w_lin = np.ascontiguousarray(state["std_feature.vn_lin.weight"], dtype=F32)
    keys = ("pos", "out1", "out2", "out3", "out4", "fstn", "local", "m", "y", "h", "trans", "e1234", "e5")
    out = {key: [] for key in keys}
    for b in range(x.shape[0]):
        pos = PN.cross_level(x[b], idx[b], fx, SLOPE)
        out1 = T.point_level(pos, fp["conv1"], SLOPE)
        out2 = T.point_level(out1, fp["conv2"], SLOPE)
        out3 = T.point_level(out2, fp["conv3"], SLOPE)
        t = out3
        for key in ("fstn.conv1", "fstn.conv2", "fstn.conv3"):
            t = T.point_level(t, fp[key], SLOPE)
        g = T.ordered_mean(t)[:, :, None]                                         # [341,3,1]: one point
        for key in ("fstn.fc1", "fstn.fc2"):
            g = T.point_level(g, fp[key], SLOPE)
        g = np.ascontiguousarray(T._chain(g, w_fc3)[0])                           # [42,3]
        out4 = T.point_level(out3, fp["conv4"], SLOPE, g=g)
        local = PN.point_norm(out4, fn)
        m = T.ordered_mean(local)
        y = T.point_level(T.point_level(local, fp["std_feature.vn1"], SLOPE, g=m), fp["std_feature.vn2"], SLOPE)
        h = T.std_pool(local, y, w_lin, g=m)[:POOLED]
        trans = np.ascontiguousarray(T.frame_rows(y, w_lin).transpose(1, 0, 2))   # [3 a, 3 k, N]
        e1234 = PS.std_coords(np.concatenate([out1, out2, out3, out4]), y, w_lin)
        e5 = PS.std_coords(local, y, w_lin)
        for key, v in zip(keys, (pos, out1, out2, out3, out4, g, local, m, y, h, trans, e1234, e5)):
            out[key].append(v)
    return {key: np.stack(v) for key, v in out.items()}


def head_f64(st, l, state, eps=1e-5):
    """The encoder's stages and l [B,16] -> logits [B,num_part,N] in float64: convs1 on the [9025,N] tensor the module builds, then
    bns1 / relu, convs2 / bns2 / relu, convs3 / bns3 / relu, convs4."""
    B, N = st["e5"].shape[0], st["e5"].shape[2]
    w_lin = state["std_feature.vn_lin.weight"]
    logits = []
    for b in range(B):
        emean = PS.std_coords(np.broadcast_to(st["m"][b][:, :, None], st["m"][b].shape + (N,)), st["y"][b], w_lin)
        const = np.concatenate([st["h"][b], np.asarray(l[b], dtype=F32)])
        net = np.concatenate([np.broadcast_to(const[:, None], (POOLED + LABEL, N)), st["e1234"][b], st["e5"][b], emean]).astype(F64)
        for i in (1, 2, 3, 4):
            w, bias = (np.asarray(state["convs%d.%s" % (i, n)], dtype=F64) for n in ("weight", "bias"))
            net = w[:, :, 0] @ net + bias[:, None]
            if i < 4:
                gamma, beta, mean, var = (np.asarray(state["bns%d.%s" % (i, n)], dtype=F64)[:, None] for n in ("weight", "bias", "running_mean", "running_var"))
                net = np.maximum((net - mean) / np.sqrt(var + eps) * gamma + beta, 0.0)
        logits.append(net)
    return np.stack(logits)
