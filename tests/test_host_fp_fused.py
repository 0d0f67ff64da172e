"""CPU tests of the fused feature-propagation level's yardstick and front end: the numpy restatement tests/fp_fused_ref.py - against
the reference's recorded eval outputs (tests/golden/fp_fused.npz) and its fp32 chain against its float64 one - the host side of the
library (svnet_fp_fused_supported, svnet_fp_fused_rows_tile, the ABI) and the argument checks of svnet_amd/fp_fused.py.  The kernel
itself: tests/test_hip_fp_fused.py."""
import os
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import fp_fused_ref as R
from tests import fused_level_cases as FL
from tests import propagate_ref as P
from tests.common import compare_case

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "fp_fused.npz"))


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_equals_the_recorded_eval_output(name):
    seed, B, N, S, D1, D2, widths = R.GOLDEN_CASES[name]
    want = GOLDEN[name + "_ev_out"]
    assert want.shape == (B, widths[-1], N) and GOLDEN[name + "_xyz1"].shape == (B, N, 3) and GOLDEN[name + "_xyz2"].shape == (B, S, 3)
    q, r, f1, f2 = R.golden_inputs(name)
    assert np.array_equal(q, GOLDEN[name + "_xyz1"]) and np.array_equal(r, GOLDEN[name + "_xyz2"]) and np.array_equal(f2, GOLDEN[name + "_points2"])
    assert (f1 is None and name + "_points1" not in GOLDEN.files) if D1 == 0 else np.array_equal(f1, GOLDEN[name + "_points1"])
    assert all(((GOLDEN["%s_sd:mlp_bns.%d.weight" % (name, i)] > 0).any() and (GOLDEN["%s_sd:mlp_bns.%d.weight" % (name, i)] < 0).any())
               for i in range(len(widths)))
    assert os.path.getsize(os.path.join(HERE, "golden", "fp_fused.npz")) < os.path.getsize(os.path.join(HERE, "golden", "msg.npz"))
    worst = compare_case({"out:new_points": R.golden_restatement(GOLDEN, name)}, {"out:new_points": want}, 1e-3, name)
    print("%s: worst relative error %.3e" % (name, worst[0]))


@pytest.mark.parametrize("S,D1,D2,widths", [(1, 0, 1, (5,)), (2, 3, 5, (12, 20)), (3, 6, 64, (33, 8, 196)), (40, 131, 1, (16, 16, 16, 7))])
def test_fp32_chain_lies_within_the_running_bound_of_the_float64_chain(S, D1, D2, widths):
    N = 21
    q, r, f2 = (a[0] for a in P.gauss_case(70 + S, 1, N, S, D2))
    f1 = synth.normal(70 + S, 6, (D1, N)) if D1 else None
    idx, _, w = P.three_nn(q, r)
    layers = FL.random_level(70 + D1, D1 + D2, widths)
    h0 = R.rows(idx, w, f2, f1)
    assert h0.dtype == F32 and h0.shape == (N, D1 + D2)
    if D1:
        assert np.array_equal(h0[:, :D1].view(np.uint32), np.ascontiguousarray(f1.T).view(np.uint32))        # the skip columns first, bit for bit
    assert np.array_equal(h0[:, D1:].view(np.uint32), np.ascontiguousarray(P.three_interpolate(f2, idx, w).T).view(np.uint32))
    got = R.level(idx, w, f2, f1, layers)
    value, bound = R.level_f64(idx, w, f2, f1, layers)
    assert got.dtype == F32 and got.shape == value.shape == bound.shape == (widths[-1], N)
    err = np.abs(got.astype(np.float64) - value)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert float(got.max()) > 0 and (bound < 1e-2 * float(value.max())).all()
    # indices outside the sampled level are clamped into it
    wild = idx.copy()
    wild[0], wild[-1] = -5, S + 9
    assert np.array_equal(R.rows(wild, w, f2, f1), R.rows(np.clip(wild, 0, S - 1), w, f2, f1))


# ---- the host side of the library
def test_supported_and_rows_tile_are_the_stated_envelope_and_the_abi_names_the_entries():
    from svnet_amd import fp_fused as FP
    # the three part-segmentation decoder levels, and the envelope's corners
    assert FP.supported(2048, 512, 22, 128, (128, 128, 128)) and FP.supported(512, 128, 128, 256, (256, 128)) and FP.supported(128, 1, 256, 1024, (256, 256))
    assert FP.supported(1, 1, 0, 1, (1,)) and FP.supported(10 ** 7, 32768, 0, 1536, (256,) * 4) and FP.supported(70, 32768, 1535, 1, (256,))
    assert FP.supported(70, 40, 512, 1024, (256, 256)) and not FP.supported(70, 40, 513, 1024, (256, 256)) and not FP.supported(70, 40, 0, 1537, (8,))
    assert FP.supported(70, 40, 3, 5, (256,)) and not FP.supported(70, 40, 3, 5, (257,)) and not FP.supported(70, 40, 3, 5, (8, 0))
    assert FP.supported(70, 40, 3, 5, (8,) * 4) and not FP.supported(70, 40, 3, 5, (8,) * 5) and not FP.supported(70, 40, 3, 5, ())
    assert FP.supported(70, 32768, 3, 5, (8,)) and not FP.supported(70, 32769, 3, 5, (8,)) and not FP.supported(70, 0, 3, 5, (8,))
    assert not FP.supported(70, 40, 8, 0, (8,)) and not FP.supported(70, 40, -1, 9, (8,)) and not FP.supported(0, 40, 3, 5, (8,))
    # rows per workgroup: the most whose two buffers fit in 160 KB; each of 64, 32 and 16 is taken somewhere
    assert FP.rows_tile(22, 128, (128, 128, 128)) == 64 and FP.rows_tile(0, 1, (5,)) == 64
    assert FP.rows_tile(132, 256, (256, 128)) == 32 and FP.rows_tile(128, 256, (256, 128)) == 32
    assert FP.rows_tile(512, 1024, (256, 256)) == 16 and FP.rows_tile(256, 1024, (256, 256)) == 16
    assert FP.rows_tile(513, 1024, (256, 256)) == 0 and FP.rows_tile(3, 5, (257,)) == 0 and FP.rows_tile(3, 0, (8,)) == 0
    for D1, D2, widths in [(22, 128, (128, 128, 128)), (132, 256, (256, 128)), (512, 1024, (256, 256)), (0, 316, (8,)), (0, 317, (8,))]:
        rows, c0 = FP.rows_tile(D1, D2, widths), D1 + D2                              # restated: strides of 4 x an odd number of floats
        ins = [c0] + list(widths[:-1])
        stride = [0, 0]
        for l, c in enumerate(ins):
            c = (c + 3) // 4 * 4
            stride[l & 1] = max(stride[l & 1], c if c % 8 else c + 4)
        assert 4 * rows * sum(stride) <= 160 * 1024 and (rows == 64 or 4 * 2 * rows * sum(stride) > 160 * 1024), (D1, D2, widths, rows)
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 429
    assert "429: svnet_fp_fused_f32, svnet_fp_fused_supported, svnet_fp_fused_rows_tile" in header
    assert "428: svnet_sa_fold_f32, svnet_sa_fused_f32" in header
    for name in ("svnet_fp_fused_f32", "svnet_fp_fused_supported", "svnet_fp_fused_rows_tile"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_fp_fused_f32"][1][4] is _lib.c_i64 and len(_lib.SIGNATURES["svnet_fp_fused_f32"][1]) == 17
    L = _lib.lib()                                                    # refused before any launch: no device is touched
    w = (_lib.c_i64 * 1)(8)
    one = (_lib.c_p * 1)(64)
    p = _lib.c_p(64)
    E = _lib.DEFINES
    assert L.svnet_fp_fused_f32(None, None, None, None, 1, 16, 4, 0, 4, 1, w, one, one, None, 8, 0, None) == E["SVNET_E_ARG"]
    assert L.svnet_fp_fused_f32(p, p, p, None, 1, 16, 4, 2, 4, 1, w, one, one, p, 8, 0, None) == E["SVNET_E_ARG"]          # D1 > 0 without points1
    assert L.svnet_fp_fused_f32(p, p, p, None, 0, 16, 4, 0, 4, 1, w, one, one, p, 8, 0, None) == E["SVNET_E_ARG"]          # B = 0
    assert L.svnet_fp_fused_f32(p, p, p, None, 1, 16, 4, 0, 1537, 1, w, one, one, p, 8, 0, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_fp_fused_f32" in L.svnet_last_error()
    assert L.svnet_fp_fused_f32(p, p, p, None, 1, 16, 4, 0, 4, 1, w, one, one, p, 8, 1, None) == E["SVNET_E_ARG"]          # c_off + 8 > 8
    assert L.svnet_fp_fused_f32(p, p, p, None, 1 << 40, 16, 4, 0, 4, 1, w, one, one, p, 8, 0, None) == E["SVNET_E_UNSUPPORTED"]       # the grid


# ---- the argument checks of the front end (no device needed: every refusal comes before the first launch)
def test_interp_mlp_refuses_bad_arguments():
    from svnet_amd import fp_fused as FP
    B, N, S, D1, D2 = 2, 16, 4, 2, 3
    idx, weight = torch.zeros(B, N, 3, dtype=torch.int64), torch.zeros(B, N, 3)
    f2, f1, level = torch.zeros(B, D2, S), torch.zeros(B, D1, N), FL.fake_level(D1 + D2, (8,))
    with pytest.raises(TypeError, match="FoldedLevel"):
        FP.interp_mlp(idx, weight, f2, f1, object())
    with pytest.raises(TypeError, match="idx must be torch.int64"):
        FP.interp_mlp(idx.int(), weight, f2, f1, level)
    with pytest.raises(TypeError, match="weight must be torch.float32"):
        FP.interp_mlp(idx, weight.double(), f2, f1, level)
    with pytest.raises(TypeError, match="points2 must be torch.float32"):
        FP.interp_mlp(idx, weight, f2.half(), f1, level)
    with pytest.raises(TypeError, match="points1 must be a tensor"):
        FP.interp_mlp(idx, weight, f2, f1.numpy(), level)
    for k in ("weight", "points2", "points1"):
        args = dict(weight=weight, points2=f2, points1=f1)
        args[k] = args[k].clone().requires_grad_()
        with pytest.raises(ValueError, match="%s requires grad" % k):
            FP.interp_mlp(idx, args["weight"], args["points2"], args["points1"], level)
    with pytest.raises(ValueError, match="points1 must be contiguous"):
        FP.interp_mlp(idx, weight, f2, torch.zeros(B, N, D1).permute(0, 2, 1), level)
    with pytest.raises(ValueError, match=r"idx and weight must be \[B,N,3\]"):
        FP.interp_mlp(idx[:, :, :2].contiguous(), weight, f2, f1, level)
    with pytest.raises(ValueError, match=r"idx and weight must be \[B,N,3\]"):
        FP.interp_mlp(idx, weight[:, :5].contiguous(), f2, f1, level)
    with pytest.raises(ValueError, match=r"points1 must be \[B,D1,N\]"):
        FP.interp_mlp(idx, weight, f2, torch.zeros(B, D1, N - 1), level)
    with pytest.raises(ValueError, match="the level takes 5 input columns, points1 and points2 give 0 \\+ 3"):
        FP.interp_mlp(idx, weight, f2, None, level)
    with pytest.raises(ValueError, match="out must be"):
        FP.interp_mlp(idx, weight, f2, f1, level, out=torch.zeros(B, 10, N), c_off=3)
    with pytest.raises(ValueError, match="out must be"):
        FP.interp_mlp(idx, weight, f2, f1, level, out=torch.zeros(B, N, 10))
    with pytest.raises(ValueError, match="c_off = 2 without out"):
        FP.interp_mlp(idx, weight, f2, f1, level, c_off=2)
    # everything in order but the device: there is no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FP.interp_mlp(idx, weight, f2, f1, level, out=torch.zeros(B, 10, N), c_off=2)


def test_the_wrapper_refuses_what_it_cannot_take():
    from svnet_amd import fp_fused as FP
    from svnet_amd.models.utils.pointnet_util import PointNetFeaturePropagation
    with pytest.raises(TypeError, match="PointNetFeaturePropagation"):
        FP.FusedFeaturePropagation(torch.nn.Linear(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FP.FusedFeaturePropagation(PointNetFeaturePropagation(12, [12, 16]))
