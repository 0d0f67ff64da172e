"""What the tests of the vector-neuron PointNet for part segmentation share (tests/test_{hip,host}_vn_pointnet_pseg.py): the golden case
of tests/golden/vn_pointnet_pseg.npz - its state, model and chained restatement - and the cases of the vector tail's wide envelope with
their references.  Every draw is a function of (seed, shape) alone and every reference is made once per process."""
import argparse

import numpy as np
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_pointnet_pseg_ref as P
from tests import vn_pointnet_ref as PN
from tests import vn_pseg_ref as PS
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import load_npz

F32 = np.float32
GOLDEN = load_npz("vn_pointnet_pseg.npz")
_once = FL.cache()
B = 2

# The wide point kernel, (C, Cg, O, Od, slope): one past the base envelope on each axis alone; vn1 and vn2 of the model; the envelope's
# corner with one direction row.  Each at N 1, 17 and 33: one tile, a tile and a tail, past two tiles - and N % 4 != 0, so x is staged
# float by float; WIDE_VEC is staged in float4s, and again float by float from a view that is not 16-byte aligned.
WIDE_POINT = [(513, 0, 4, 4, 0.2), (4, 0, 513, 513, 0.2), (4, 513, 4, 4, 0.2), (682, 682, 682, 682, 0.0), (768, 768, 768, 1, 0.2), (682, 0, 341, 341, 0.0)]
WIDE_POINT_N = [1, 17, 33]
WIDE_VEC = (682, 0, 341, 341, 0.0, 80)
# the wide norm-only layer, (C, O): the model's conv5 + bn5 and the corner
WIDE_NORM = [(170, 682), (768, 768)]
WIDE_NORM_N = [17, 65]
# the wide mean and pool: a single run, an exact run, a run plus one, three runs with a short last one
RUN_N = [1, 64, 65, 130]
WIDE_MEAN_C = 682
WIDE_STD = [(513, 0, 4), (4, 513, 4), (4, 0, 513), (682, 682, 341), (768, 768, 768)]          # (C, Cg, Cy): 1364 columns are 21 slabs and one of 20
WIDE_COORDS = [(682, 341), (768, 768)]                                                       # (C, Cy) at N 65
# Old against new, (C, Cg, O, Od, N): shapes both envelopes admit.  The widest O of the base envelope over vn1's 341 + 341 inputs (two
# workgroups a CU), and the base envelope's corner (one).
BOTH = [(341, 341, 512, 512, 65), (512, 512, 512, 1, 17)]


def point_arrays(C, Cg, O, Od, N):
    def make():
        seed = 9700 + 13 * C + 7 * Cg + O
        return synth.normal(seed, 1, (B, C, 3, N)), synth.normal(seed, 2, (B, Cg, 3)), VC.layer_arrays(seed, C + Cg, O, Od, signs=7)
    return _once(("point arrays", C, Cg, O, Od, N), make)


def point_want(C, Cg, O, Od, N, slope):
    def make():
        x, g, a = point_arrays(C, Cg, O, Od, N)
        f = T.fold_point(a["w_feat"], a["w_dir"], a["gamma"], a["beta"], a["mean"], a["var"])
        return f, np.stack([T.point_level(x[b], f, slope, g[b] if Cg else None) for b in range(B)])
    return _once(("point want", C, Cg, O, Od, N, slope), make)


def norm_arrays(C, O, N):
    def make():
        seed = 9800 + 11 * C + O
        return synth.normal(seed, 1, (B, C, 3, N)), VC.layer_arrays(seed, C, O, O)
    return _once(("norm", C, O, N), make)


def norm_want(C, O, N):
    def make():
        x, a = norm_arrays(C, O, N)
        f = PN.fold_norm(a["w_feat"], a["gamma"], a["beta"], a["mean"], a["var"])
        return f, np.stack([PN.point_norm(x[b], f) for b in range(B)])
    return _once(("norm want", C, O, N), make)


def std_arrays(C, Cg, Cy, N, want=True):
    """(x, g, y, w_lin, the pool's h or None, the ordered mean of x)."""
    def make():
        seed = 9900 + 11 * C + 5 * Cg + Cy + N
        x, g = synth.normal(seed, 1, (B, C, 3, N)), synth.normal(seed, 2, (B, Cg, 3))
        y, w_lin = synth.normal(seed, 3, (B, Cy, 3, N)), (synth.normal(seed, 4, (3, Cy)) / np.sqrt(F32(Cy))).astype(F32)
        h = np.stack([T.std_pool(x[b], y[b], w_lin, g[b] if Cg else None) for b in range(B)]) if want else None
        return x, g, y, w_lin, h, T.ordered_mean(x)
    return _once(("std", C, Cg, Cy, N, want), make)


def coords_want(C, Cy, N):
    def make():
        x, _, y, w_lin, _, _ = std_arrays(C, 0, Cy, N, want=False)
        return np.stack([PS.std_coords(x[b], y[b], w_lin) for b in range(B)])
    return _once(("coords", C, Cy, N), make)


def state():
    return _once("state", lambda: V.synthetic_state(GOLDEN["keys"], GOLDEN["shapes"], P.GOLDEN_CASE[0]))


def golden_model(dev=None, pooling="mean"):
    import svnet_amd.models as M
    seed, _, N, k, num_part = P.GOLDEN_CASE
    model = M.VN_PointNet_PSEG(argparse.Namespace(k=k, pooling=pooling), num_part)
    if pooling == "mean":
        model.load_state_dict({key: torch.from_numpy(np.array(v)) for key, v in state().items()}, strict=True)
    return model.to(dev).eval()


def restated():
    """The chained restatement of the fused forward on the golden case: {stage: array}, the float64 head's logits among them."""
    def make():
        st = P.encoder(GOLDEN["x"], GOLDEN["idx"], state())
        st["logits"] = P.head_f64(st, GOLDEN["l"], state())
        return st
    return _once("restated", make)
