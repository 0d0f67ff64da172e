"""GPU tests (-m gpu): k-NN past the register-resident range - 4096 < N <= 32768 or 64 < k <= 128 - which the streamed kernel
(csrc/knn.hip, knn_stream_kernel) takes, and the models at those sizes.

k-NN indices are compared element for element with the exact oracle: both break exactly tied distances by the lowest index.
"""

import numpy as np
import pytest
import torch

from oracle import knn as oknn
from oracle import params as oparams
from oracle import sv_ref
from svnet_amd import synth
from tests.decisions import decisions_of, tapped
from tests.golden import cases as C

pytestmark = pytest.mark.gpu


def _input(B, N, Cc, layout, tag):
    """A [B,C,N] tensor as the reference's knn() receives it: the cloud itself (layout "cn", C = 3) or a transposed view of [B,N,C]."""
    sid = synth.stream_id("knn_large/%s" % tag)
    if layout == "cn":
        return torch.from_numpy(synth.cloud_batch(C.SEED, 11, sid % 1000, B, N))
    return torch.from_numpy(synth.normal(C.SEED, sid, (B, N, Cc)) * 0.7).transpose(-1, -2)


def _on(x, dev):
    """The same tensor on the device, with the same strides."""
    if x.is_contiguous():
        return x.to(dev)
    return x.transpose(-1, -2).contiguous().to(dev).transpose(-1, -2)


# (B, N, C, k, layout): a sample of N in {4097, 6000, 8192, 12288, 16384} x C in {3 cn, 20, 62, 127, 136, 384} x k in {20, 40, 64, 65, 100,
# 128}, B = 1, 2 and 8 (the XCD-aware cloud order), one N = 32768, and k > 64 at N <= 4096
SHAPES = [
    (2, 4097, 3, 20, "cn"), (1, 4097, 62, 65, "nc"), (2, 6000, 20, 40, "nc"), (1, 6000, 127, 100, "nc"), (1, 6000, 384, 20, "nc"),
    (2, 8192, 3, 20, "cn"), (2, 8192, 62, 20, "nc"), (1, 8192, 127, 40, "nc"), (1, 8192, 136, 64, "nc"), (1, 8192, 20, 128, "nc"),
    (8, 8192, 3, 20, "cn"), (8, 4608, 62, 40, "nc"),
    (1, 12288, 20, 100, "nc"), (1, 12288, 3, 65, "cn"), (1, 16384, 3, 20, "cn"), (1, 16384, 62, 40, "nc"), (1, 16384, 20, 128, "nc"),
    (1, 32768, 3, 20, "cn"),
    (2, 65, 12, 65, "nc"), (3, 100, 7, 100, "nc"), (2, 1024, 62, 128, "nc"), (1, 4096, 127, 128, "nc"), (8, 1024, 62, 80, "nc"),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["B%d_N%d_C%d_k%d_%s" % s for s in SHAPES])
def test_knn_large_bit_exact(shape, hip_device):
    from svnet_amd.models.utils.sv_util import knn
    B, N, Cc, k, layout = shape
    x = _input(B, N, Cc, layout, "%d_%d_%d" % (N, Cc, k))
    xd = _on(x, hip_device)
    assert xd.stride() == x.stride()
    got = knn(xd, k).cpu()
    assert got.shape == (B, N, k)
    ref = oknn.knn_exact(x, k)
    assert int((got != ref).sum()) == 0


@pytest.mark.parametrize("k,dup,at", [(40, 150, 40), (128, 400, 20), (40, 150, 8000), (128, 200, 4000)])
def test_knn_large_heavy_ties(k, dup, at, hip_device):
    """`dup` copies of one point, placed from index `at` on so that they straddle the 64-candidate chunks of the streamed kernel (and,
    at `at` = 20, fill the first chunk with more tied candidates than one chunk has lanes); the lowest index wins every tie."""
    from svnet_amd.models.utils.sv_util import knn
    N = 8192
    feat = torch.from_numpy(synth.normal(C.SEED, synth.stream_id("knn_large_dup/%d_%d" % (k, dup)), (2, N, 20)) * 0.7)
    feat[0, at:at + dup] = feat[0, at]
    feat[1, N - dup:] = feat[1, 3]
    feat[1, 3 + 64] = feat[1, 3]
    x = feat.transpose(-1, -2)
    got = knn(feat.to(hip_device).transpose(-1, -2), k).cpu()
    ref = oknn.knn_exact(x, k)
    assert int((got != ref).sum()) == 0
    # the copies' own lists: k tied candidates at distance 0, lowest indices first
    assert got[0, at + 1, :k].tolist() == list(range(at, at + k))


@pytest.mark.parametrize("Cs,Cv,k", [(21, 21, 20), (42, 28, 80)])
def test_knn_sv_large(Cs, Cv, k, hip_device):
    """The two-source feature graph (get_graph_feature_sv) at N = 8192: rows cat[s, v.view(B,N,3Cv)] read from strided s [B,N,Cs] and
    v [B,N,3,Cv], equal to the exact oracle on the concatenated rows."""
    from svnet_amd import _ops
    B, N = 2, 8192
    sid = synth.stream_id("knn_large_sv/%d_%d" % (Cs, Cv))
    s_big = torch.from_numpy(synth.normal(C.SEED, sid, (B, N, Cs + 5)) * 0.7)
    v = torch.from_numpy(synth.normal(C.SEED, sid + 1, (B, N, 3, Cv)) * 0.7)
    s = s_big[:, :, 2:2 + Cs]                                         # strided: a slice of wider rows
    rows = torch.cat([s, v.reshape(B, N, 3 * Cv)], dim=-1)
    ref = oknn.knn_exact(rows.transpose(-1, -2), k)
    got = _ops.knn_sv(s_big.to(hip_device)[:, :, 2:2 + Cs], v.to(hip_device), k).cpu()
    assert int((got != ref).sum()) == 0


# (tag, model, binary, B, N, k): the callers at --num-points past 4096 and at --k past 64
EVAL_CASES = [
    ("large_dgcnn_bin_n8192", "sv_dgcnn_cls", True, 2, 8192, 20),      # the fused edge path past 4096 points
    ("large_dgcnn_fp_n8192", "sv_dgcnn_cls", False, 2, 8192, 20),
    ("large_dgcnn_fp_n16384", "sv_dgcnn_cls", False, 1, 16384, 20),    # layer-wise edges past the fused path's 8192 points
    ("large_pseg_bin_k80", "sv_dgcnn_pseg", True, 1, 2048, 80),        # layer-wise edges at k > 64
    ("large_pointnet_bin_n8192", "sv_pointnet_cls", True, 2, 8192, 20),
]


@pytest.mark.parametrize("case", EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_models_eval_large_match_oracle(case, hip_device):
    """Eval-mode logits of the whole model against the oracle with the HIP run's discrete decisions replayed (tests/decisions.py),
    element-wise at 1e-3 of the logit range - as test_hip_parity.test_models_eval_match_golden, without its golden leg."""
    from tests.golden import harness as H
    from tests.test_hip_parity import _build, _oracle_forward
    tag, model, binary, B, N, k = case
    P = oparams.synthetic_params(model, binary=binary, seed=C.SEED)
    x, l, _ = C.model_inputs(tag, model, B, N)
    m = _build(model, binary, k, hip_device, P).eval()
    with tapped() as tap, torch.no_grad():
        out = (m(x.to(hip_device), l.to(hip_device)) if l is not None else m(x.to(hip_device))).cpu().numpy()
    # a binary model's features are popcounts: at 8192 points a cloud holds many candidates at nearly equal distance, and the oracle's
    # own fp32 rounding re-orders up to ~1.3 % of the feature-space neighbour slots (measured at B = 2, N = 8192: 4 229 of 327 680, every
    # one certified as a knife edge within 6 % of the certificate's bound); the kernel itself is held bit-exact on given features above
    kw = {"max_fraction": 2e-2} if binary else {}
    with torch.no_grad():
        dec64 = decisions_of(tap, **kw)
        dec64.value_record = {"knn": [], "signs": [], "pools": []}
        ctx64 = sv_ref.Ctx(train=False)
        ctx64.decisions = dec64
        P64 = {n: (t.double() if t.is_floating_point() else t) for n, t in P.items()}
        _oracle_forward(model, binary, k, x.double(), None if l is None else l.double(), P64, ctx64)
        dec = decisions_of(tap, **kw)
        dec.truth = dec64.value_record
        ctx = sv_ref.Ctx(train=False)
        ctx.decisions = dec
        lo = _oracle_forward(model, binary, k, x, l, P, ctx).numpy()
    cert = dec.check()
    assert np.isfinite(out).all()
    assert H.max_rel_err(out, lo) < 1e-3, (H.max_rel_err(out, lo), cert)


# the train step past 4096 points (fused forward and backward, reverse lists of more than 4096 points) and at k > 64 (layer-wise)
TRAIN_CASES = [
    ("large_dgcnn_bin_n4608", "sv_dgcnn_cls", True, 2, 4608, 20),
    ("large_dgcnn_bin_k80", "sv_dgcnn_cls", True, 8, 128, 80),
]


@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_train_step_large_matches_oracle(case, hip_device):
    """Loss, logits and every parameter gradient of one train step against the oracle, element-wise, with the HIP run's decisions
    replayed - test_hip_train_parity.test_train_step_matches_oracle_elementwise's comparison at the new sizes."""
    from tests.test_hip_train_parity import _train_step_case
    _train_step_case(case, hip_device)
