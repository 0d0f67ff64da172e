"""CPU tests of the fused set-abstraction level's yardstick and front end: the numpy restatement tests/sa_fused_ref.py - its exact
fmaf against rational arithmetic, its fp32 chain against its float64 one, and both against the reference's recorded eval outputs
(tests/golden/msg.npz, tests/golden/sa_fused.npz) - the host side of the library (svnet_sa_fused_supported, the ABI) and the argument
checks of svnet_amd/sa_fused.py.  The kernels themselves: tests/test_hip_sa_fused.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import fused_level_cases as FL
from tests import msg_ref as M
from tests import sa_fused_ref as R
from tests.common import compare_case

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MSG = np.load(os.path.join(HERE, "golden", "msg.npz"))
GOLDEN = np.load(os.path.join(HERE, "golden", "sa_fused.npz"))


def _round_f32(q):
    """The fp32 nearest to the rational q, ties to the even mantissa: the nearest of the double-rounded guess and its two neighbours."""
    g = F32(float(q))
    cands = [g, np.nextafter(g, F32(-np.inf)), np.nextafter(g, F32(np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.array(v).view(np.uint32)) & 1))
    return best


def _exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf_equals_rational_arithmetic_on_random_operands():
    n = 3000
    a = synth.normal(3, 1, (n,)) * np.exp2(synth.integers(3, 2, (n,), 40) - 20).astype(F32)
    b = synth.normal(3, 3, (n,)) * np.exp2(synth.integers(3, 4, (n,), 40) - 20).astype(F32)
    c = synth.normal(3, 5, (n,)) * np.exp2(synth.integers(3, 6, (n,), 40) - 20).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3])).astype(F32)              # cancellation: the sum is the product's own rounding error
    c[1::7] = 0
    got = R.fmaf(a, b, c)
    assert got.dtype == F32 and got.shape == (n,)
    want = np.array([_exact(*v) for v in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fmaf_is_right_where_float64_arithmetic_rounds_twice():
    """(1 + x)(1 - x) = 1 - x^2 with x = 2^-k, 15 <= k <= 23, added to c = 2^24 + 2 (ulp 2, odd mantissa): the exact sum 2^24 + 3 - x^2
    lies just BELOW the tie 2^24 + 3 and rounds to c; float64 cannot hold x^2 <= 2^-30 beside 2^24, lands on the tie and rounds to the
    even neighbour 2^24 + 4.  The mirrored case and scalings by powers of two likewise."""
    a, b, c = [], [], []
    for k in range(15, 24):
        for scale in (1.0, 2.0 ** 10, 2.0 ** -30):
            for sign in (1.0, -1.0):
                a.append(sign * (1 + 2.0 ** -k) * scale)
                b.append(1 - 2.0 ** -k)
                c.append(sign * (2.0 ** 24 + 2) * scale)
    a, b, c = (np.array(v, dtype=np.float64) for v in (a, b, c))
    assert all(np.array_equal(v, v.astype(F32).astype(np.float64)) for v in (a, b, c))         # fp32 operands
    a, b, c = a.astype(F32), b.astype(F32), c.astype(F32)
    want = np.array([_exact(*v) for v in zip(a, b, c)], dtype=F32)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (naive != want).all(), "the constructed cases do not round twice"
    assert np.array_equal(want, c)
    assert np.array_equal(R.fmaf(a, b, c).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("C0,widths,K,xyz_last", [(3, (5,), 1, False), (7, (12, 20), 9, True), (67, (33, 8, 196), 4, False),
                                                  (131, (16, 16, 16, 7), 3, True)])
def test_fp32_chain_lies_within_the_running_bound_of_the_float64_chain(C0, widths, K, xyz_last):
    N, S, D = 40, 5, C0 - 3
    x = (synth.normal(8, 1, (N, 3)) * F32(0.5)).astype(F32)
    c = np.ascontiguousarray(x[:S] + F32(0.01))
    pts = synth.normal(8, 2, (N, D)) if D else None
    idx = synth.integers(8, 3, (S, K), N).astype(np.int64)
    layers = FL.random_level(8 + C0, C0, widths)
    got = R.level(x, c, idx, pts, layers, xyz_last)
    value, bound = R.level_f64(x, c, idx, pts, layers, xyz_last)
    assert got.dtype == F32 and got.shape == value.shape == bound.shape == (widths[-1], S)
    err = np.abs(got.astype(np.float64) - value)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    # the bound says something: it grows by sum |Wf| per layer, and after four layers is still under a hundredth of the largest output
    assert float(got.max()) > 0 and (bound < 1e-2 * float(value.max())).all()
    # the fold: against float64 arithmetic within four roundings, and the sign of a negative BatchNorm weight carried into Wf
    s0 = FL.layer_state(8 + C0, C0, widths)[0]
    scale = s0["gamma"].astype(np.float64) / np.sqrt(s0["var"].astype(np.float64) + 1e-5)
    Wf, bf = layers[0]
    assert np.allclose(Wf, s0["W"] * scale[:, None], rtol=4 * 2.0 ** -23, atol=0) and (s0["gamma"] < 0).any()
    assert np.allclose(bf, (s0["b"].astype(np.float64) - s0["mean"]) * scale + s0["beta"], rtol=0, atol=1e-6)


def _msg_restatement(name):
    seed, B, N, S, radii, nsamples, D, mlp_list = M.GOLDEN_CASES[name]
    state = {str(k): MSG["%s_sd:%s" % (name, k)] for k in MSG[name + "_keys"]}
    x, c = MSG[name + "_xyz"], MSG[name + "_new_xyz"]
    pts = MSG[name + "_points"] if D else None
    outs = []
    for i, mlp in enumerate(mlp_list):
        layers = R.fold_state(state, R.msg_prefixes(i, len(mlp)))
        outs.append(R.level_batch(x, c, MSG["%s_idx%d" % (name, i)].astype(np.int64), pts, layers, xyz_last=True))
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("name", list(M.GOLDEN_CASES))
def test_restatement_equals_the_recorded_multi_scale_eval_outputs(name):
    want = MSG[name + "_ev_out:new_points"]
    got = _msg_restatement(name)
    worst = compare_case({"out:new_points": got}, {"out:new_points": want}, 1e-3, name)
    print("%s: worst relative error %.3e" % (name, worst[0]))


def golden_single():
    seed, B, N, S, radius, nsample, D, mlp = R.GOLDEN_CASE
    state = {str(k): GOLDEN["sd:" + str(k)] for k in GOLDEN["keys"]}
    layers = R.fold_state(state, R.single_prefixes(len(mlp)))
    return R.level_batch(GOLDEN["xyz"], GOLDEN["new_xyz"], GOLDEN["idx"].astype(np.int64), GOLDEN["points"], layers)


def test_restatement_equals_the_recorded_single_scale_eval_output():
    seed, B, N, S, radius, nsample, D, mlp = R.GOLDEN_CASE
    want = GOLDEN["ev_out:new_points"]
    assert want.shape == (B, mlp[-1], S) and GOLDEN["xyz"].shape == (B, N, 3) and GOLDEN["points"].shape == (B, N, D)
    x, pts = R.golden_inputs()
    assert np.array_equal(x, GOLDEN["xyz"]) and np.array_equal(pts, GOLDEN["points"])
    assert all(((GOLDEN["sd:mlp_bns.%d.weight" % i] > 0).any() and (GOLDEN["sd:mlp_bns.%d.weight" % i] < 0).any()) for i in range(len(mlp)))
    assert os.path.getsize(os.path.join(HERE, "golden", "sa_fused.npz")) < os.path.getsize(os.path.join(HERE, "golden", "msg.npz"))
    worst = compare_case({"out:new_points": golden_single()}, {"out:new_points": want}, 1e-3, "sa_fused.npz")
    print("worst relative error %.3e" % worst[0])


# ---- the host side of the library
def test_supported_is_the_stated_envelope_and_the_abi_names_the_entries():
    from svnet_amd import sa_fused as SF
    assert SF.rows_tile() >= 16 and SF.rows_tile() % 16 == 0
    assert SF.supported(1024, 512, 32, 0, (64, 64, 128)) and SF.supported(512, 128, 64, 128, (128, 128, 256))
    assert SF.supported(1024, 512, 128, 0, (64, 96, 128)) and SF.supported(512, 128, 16, 320, (196, 3)) and SF.supported(64, 1, 1, 320, (256,) * 4)
    assert SF.supported(32768, 1, 32768, 0, (5,)) and SF.supported(1, 1, 1, 0, (1,))
    for bad in [(16, 4, 17, 0, (8,)), (32769, 4, 8, 0, (8,)), (16, 0, 4, 0, (8,)), (16, 4, 0, 0, (8,)), (16, 4, 4, -1, (8,)), (16, 4, 4, 322, (8,)),
                (16, 4, 4, 0, (257,)), (16, 4, 4, 0, (8, 0)), (16, 4, 4, 0, ()), (16, 4, 4, 0, (8,) * 5)]:
        assert not SF.supported(*bad), bad
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 428 and "428: svnet_sa_fold_f32, svnet_sa_fused_f32" in header
    for name in ("svnet_sa_fold_f32", "svnet_sa_fused_f32", "svnet_sa_fused_supported", "svnet_sa_fused_rows_tile"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_sa_fused_f32"][1][4] is _lib.c_i64 and _lib.SIGNATURES["svnet_sa_fold_f32"][1][8] is _lib.c_f
    assert _lib.DEFINES["SVNET_SA_MAX_LAYERS"] == SF.MAX_LAYERS == 4
    L = _lib.lib()                                                    # refused before any launch: no device is touched
    w = (_lib.c_i64 * 1)(8)
    one = (_lib.c_p * 1)(64)
    assert L.svnet_sa_fused_f32(None, None, None, None, 4, None, 0, 1, 16, 4, 4, 0, 1, w, one, one, 0, None, 8, 0, None) == _lib.DEFINES["SVNET_E_ARG"]
    p = _lib.c_p(64)
    assert L.svnet_sa_fused_f32(p, p, None, p, 4, None, 0, 1, 16, 4, 17, 0, 1, w, one, one, 0, p, 8, 0, None) == _lib.DEFINES["SVNET_E_UNSUPPORTED"]
    assert b"svnet_sa_fused_f32" in L.svnet_last_error()
    assert L.svnet_sa_fused_f32(p, p, None, p, 3, None, 0, 1, 16, 4, 4, 0, 1, w, one, one, 0, p, 8, 0, None) == _lib.DEFINES["SVNET_E_ARG"]     # idx_ld < K
    assert L.svnet_sa_fused_f32(p, p, None, p, 4, None, 0, 1, 16, 4, 4, 0, 1, w, one, one, 0, p, 8, 1, None) == _lib.DEFINES["SVNET_E_ARG"]     # c_off + 8 > 8
    assert L.svnet_sa_fold_f32(p, p, p, p, p, None, 4, 4, 1e-5, p, p, None) == _lib.DEFINES["SVNET_E_ARG"]
    assert L.svnet_sa_fold_f32(p, p, p, p, p, p, 0, 4, 1e-5, p, p, None) == _lib.DEFINES["SVNET_E_ARG"]


# ---- the argument checks of the front end (no device needed: every refusal comes before the first launch)
def test_group_mlp_max_refuses_bad_arguments():
    from svnet_amd import sa_fused as SF
    B, N, S, K, D = 2, 16, 4, 4, 2
    xyz, new_xyz, pts = torch.zeros(B, N, 3), torch.zeros(B, S, 3), torch.zeros(B, N, D)
    idx, count, level = torch.zeros(B, S, K, dtype=torch.int64), torch.ones(B, S, dtype=torch.int32), FL.fake_level(3 + D, (8,))
    with pytest.raises(TypeError, match="FoldedLevel"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, object())
    with pytest.raises(TypeError, match="idx must be torch.int64"):
        SF.group_mlp_max(xyz, new_xyz, idx.int(), pts, level)
    with pytest.raises(TypeError, match="count must be torch.int32"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, level, count=count.long())
    with pytest.raises(TypeError, match="xyz must be torch.float32"):
        SF.group_mlp_max(xyz.double(), new_xyz, idx, pts, level)
    with pytest.raises(TypeError, match="points must be a tensor"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts.numpy(), level)
    for k in ("xyz", "new_xyz", "points"):
        args = dict(xyz=xyz, new_xyz=new_xyz, points=pts)
        args[k] = args[k].clone().requires_grad_()
        with pytest.raises(ValueError, match="%s requires grad" % k):
            SF.group_mlp_max(args["xyz"], args["new_xyz"], idx, args["points"], level)
    with pytest.raises(ValueError, match="xyz must be contiguous"):
        SF.group_mlp_max(torch.zeros(B, 3, N).permute(0, 2, 1), new_xyz, idx, pts, level)
    with pytest.raises(ValueError, match=r"new_xyz must be \[B,S,3\]"):
        SF.group_mlp_max(xyz, new_xyz[:1], idx, pts, level)
    with pytest.raises(ValueError, match=r"idx must be \[B,S,K\]"):
        SF.group_mlp_max(xyz, new_xyz, idx[:, :2], pts, level)
    with pytest.raises(ValueError, match="idx must be contiguous, or a slice of the last axis"):
        SF.group_mlp_max(xyz, new_xyz, torch.zeros(B, K, S, dtype=torch.int64).permute(0, 2, 1), pts, level)
    with pytest.raises(ValueError, match="idx must be contiguous, or a slice of the last axis"):
        SF.group_mlp_max(xyz, new_xyz, torch.zeros(B, S, 2 * K, dtype=torch.int64)[:, :, ::2], pts, level)
    with pytest.raises(ValueError, match=r"count must be \[B,S\]"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, level, count=count[:, :2])
    with pytest.raises(ValueError, match=r"points must be \[B,N,D\]"):
        SF.group_mlp_max(xyz, new_xyz, idx, torch.zeros(B, N - 1, D), level)
    with pytest.raises(ValueError, match="the level takes 5 input columns"):
        SF.group_mlp_max(xyz, new_xyz, idx, None, level)
    with pytest.raises(ValueError, match="out must be"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, level, out=torch.zeros(B, 10, S), c_off=3)
    with pytest.raises(ValueError, match="out must be"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, level, out=torch.zeros(B, S, 10))
    with pytest.raises(ValueError, match="c_off = 2 without out"):
        SF.group_mlp_max(xyz, new_xyz, idx, pts, level, c_off=2)
    # everything in order but the device: there is no CPU fallback; a slice of a concatenated table passes the stride check
    wide, counts = torch.zeros(B, S, 3 * K, dtype=torch.int64), torch.ones(B, S, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.group_mlp_max(xyz, new_xyz, wide[:, :, K:2 * K], pts, level, count=counts[:, :, 1], out=torch.zeros(B, 10, S), c_off=2)


def test_fold_level_and_the_wrapper_refuse_what_they_cannot_take():
    from svnet_amd import sa_fused as SF
    from svnet_amd.models.utils.pointnet_msg import PointNetSetAbstractionMsg
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    convs = [torch.nn.Conv2d(5, 8, 1), torch.nn.Conv2d(8, 6, 1)]
    bns = [torch.nn.BatchNorm2d(8), torch.nn.BatchNorm2d(6)]
    with pytest.raises(ValueError, match="needs 1 .. 4 pairs"):
        SF.fold_level(convs, bns[:1])
    with pytest.raises(ValueError, match="needs 1 .. 4 pairs"):
        SF.fold_level([], [])
    with pytest.raises(ValueError, match="1x1 convolution with a bias"):
        SF.fold_level([torch.nn.Conv2d(5, 8, 3)], bns[:1])
    with pytest.raises(ValueError, match="1x1 convolution with a bias"):
        SF.fold_level([torch.nn.Conv2d(5, 8, 1, bias=False)], bns[:1])
    with pytest.raises(ValueError, match="behind a layer of width 8"):
        SF.fold_level([convs[0], torch.nn.Conv2d(7, 6, 1)], bns)
    with pytest.raises(ValueError, match="track running statistics"):
        SF.fold_level(convs[:1], [torch.nn.BatchNorm2d(8, track_running_stats=False)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.fold_level(convs, bns)
    with pytest.raises(TypeError, match="PointNetSetAbstraction"):
        SF.FusedSetAbstraction(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="group_all"):
        SF.FusedSetAbstraction(PointNetSetAbstraction(None, None, None, 7, [8], True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.FusedSetAbstraction(PointNetSetAbstraction(4, 0.2, 4, 7, [8], False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.FusedSetAbstraction(PointNetSetAbstractionMsg(4, [0.2, 0.4], [4, 8], 4, [[8], [8, 6]]))
