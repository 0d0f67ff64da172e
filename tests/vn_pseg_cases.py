"""What the tests of the part-segmentation vector-neuron model share (tests/test_{hip,host}_vn_pseg.py): the golden case of
tests/golden/vn_pseg.npz - its state, model, recorded levels and lists - and the restated tail in front of the coordinates.  Every
reference is made once per process."""
import argparse

import numpy as np
import torch

from tests import fused_level_cases as FL
from tests import vn_pseg_ref as P
from tests import vn_tail_ref as T
from tests.common import load_npz

F32 = np.float32
GOLDEN = load_npz("vn_pseg.npz")
_once = FL.cache()


def state():
    return _once("state", lambda: P.pseg_state(GOLDEN["keys"], GOLDEN["shapes"], P.GOLDEN_CASE[0]))


def golden_model(dev=None, pooling="mean"):
    import svnet_amd.models as M
    seed, B, N, k, num_part = P.GOLDEN_CASE
    model = M.VN_DGCNN_PSEG(argparse.Namespace(k=k, pooling=pooling), num_part)
    if pooling == "mean":
        model.load_state_dict({key: torch.from_numpy(np.array(v)) for key, v in state().items()}, strict=True)
    return model.to(dev).eval()


def levels():
    return [GOLDEN["lvl%d" % i] for i in range(3)]


def lists():
    return [GOLDEN["idx%d" % i] for i in range(3)]


def frame_inputs():
    """(x123 [B,63,3,N], y [B,170,3,N]): the recorded levels and the restated conv6 -> vn1 -> vn2 on them, what the coordinates read."""
    def make():
        st = state()
        x123 = np.concatenate(levels(), axis=1)
        f6, fv1, fv2 = (T.fold_point_state(st, p) for p in ("conv6.", "std_feature.vn1.", "std_feature.vn2."))
        ys = []
        for b in range(x123.shape[0]):
            local = T.point_level(x123[b], f6)
            ys.append(T.point_level(T.point_level(local, fv1, g=T.ordered_mean(local)), fv2))
        return x123, np.stack(ys)
    return _once("frame inputs", make)
