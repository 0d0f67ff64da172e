"""What the tests of the vector-neuron PointNet share (tests/test_{hip,host}_vn_pointnet.py): the golden case of
tests/golden/vn_pointnet.npz - its state and model - the synthetic layers of the position level and of the norm-only point layer,
and the case lists.  Every draw is a function of (seed, shape) alone and every reference is made once per process."""
import argparse

import numpy as np
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_pointnet_ref as P
from tests import vn_ref as V
from tests.common import load_npz

F32 = np.float32
GOLDEN = load_npz("vn_pointnet.npz")
_once = FL.cache()
KEYS = ("w_feat", "w_dir", "gamma", "beta", "mean", "var")

# The position level, (B, N, k, O, share, slope, lists).  The self edge (N = k = 1: difference and cross product are zero); three points
# that are each other's neighbours; k at its limit with N across a wave; three clouds, N across two waves and no multiple of 64, the
# model's width; one channel; the widest level (16 chunks of 8 channels); one direction row; the other slope at a width that is no
# multiple of the chunk; entries -1 and N + 5, which are clamped.
CROSS_CASES = [(1, 1, 1, 21, False, 0.0, "random"),
               (1, 3, 3, 21, False, 0.0, "random"),
               (2, 65, 64, 21, False, 0.0, "random"),
               (3, 130, 20, 21, False, 0.0, "random"),
               (2, 33, 5, 1, False, 0.0, "random"),
               (2, 33, 5, 128, False, 0.2, "random"),
               (2, 33, 5, 21, True, 0.0, "random"),
               (2, 33, 5, 7, False, 0.2, "random"),
               (2, 33, 5, 21, False, 0.0, "outside")]
# the host's cases against float64: (N, k, O, Od, slope)
CROSS_HOST_CASES = [(33, 5, 7, 7, 0.0), (33, 5, 7, 7, 0.2), (33, 5, 7, 1, 0.0), (33, 5, 7, 1, 0.2)]
# the norm-only point layer: (C, O) x N at B 2
NORM_WIDTHS = [(1, 1), (42, 341), (5, 17)]
NORM_POINTS = [1, 17, 130]


def cross_arrays(B, N, k, O, share, lists="random"):
    """(x [B,1,3,N], idx [B,N,k], the layer's arrays) of a position level."""
    def make():
        seed = 9100 + 7 * O + N
        x = synth.normal(seed, 1, (B, 1, 3, N))
        idx = synth.integers(seed, 2, (B, N, k), N)
        if lists == "outside":
            idx = idx.copy()
            idx[:, ::2, 0], idx[:, 1::2, -1] = -1, N + 5
        return x, idx, VC.layer_arrays(seed, 3, O, 1 if share else O)
    return _once(("cross", B, N, k, O, share, lists), make)


def cross_want(B, N, k, O, share, slope, lists="random"):
    def make():
        x, idx, a = cross_arrays(B, N, k, O, share, lists)
        f = P.fold_cross(*(a[key] for key in KEYS))
        return f, P.cross_level_batch(x, idx, f, slope)
    return _once(("cross want", B, N, k, O, share, slope, lists), make)


def norm_arrays(C, O, N, B=2):
    def make():
        seed = 9300 + 11 * C + O
        return synth.normal(seed, 1, (B, C, 3, N)), VC.layer_arrays(seed, C, O, O)
    return _once(("norm", C, O, N, B), make)


def norm_want(C, O, N, B=2):
    def make():
        x, a = norm_arrays(C, O, N, B)
        f = P.fold_norm(a["w_feat"], a["gamma"], a["beta"], a["mean"], a["var"])
        return f, np.stack([P.point_norm(x[b], f) for b in range(B)])
    return _once(("norm want", C, O, N, B), make)


def norm_layers(dev, C, O, a):
    """(VNLinear, VNBatchNorm) over C -> O that hold the arrays a, on dev in eval mode."""
    from svnet_amd.models.vn_layers import VNBatchNorm, VNLinear
    linear, norm = VNLinear(C, O), VNBatchNorm(O, dim=4)
    with torch.no_grad():
        for t, key in ((linear.map_to_feat.weight, "w_feat"), (norm.bn.weight, "gamma"), (norm.bn.bias, "beta"), (norm.bn.running_mean, "mean"),
                       (norm.bn.running_var, "var")):
            t.copy_(torch.from_numpy(a[key]))
    return linear.to(dev).eval(), norm.to(dev).eval()


def state():
    return _once("state", lambda: V.synthetic_state(GOLDEN["keys"], GOLDEN["shapes"], P.GOLDEN_CASE[0]))


def golden_model(dev=None, pooling="mean"):
    import svnet_amd.models as M
    seed, B, N, k, num_class = P.GOLDEN_CASE
    model = M.VN_PointNet_CLS(argparse.Namespace(k=k, pooling=pooling), num_class)
    if pooling == "mean":
        model.load_state_dict({key: torch.from_numpy(np.array(v)) for key, v in state().items()}, strict=True)
    return model.to(dev).eval()


def restated():
    """The chained restatement of the encoder on the golden case: {stage: array}."""
    return _once("restated", lambda: P.encoder(GOLDEN["x"], GOLDEN["idx"], state()))
