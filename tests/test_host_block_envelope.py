"""CPU tests of the fused blocks' shape envelope (no GPU): the launch ladders as host functions (svnet_edgeblock_fwd_tier,
svnet_edgeblock_bwd_tier, svnet_edgeblock_wgrad_tier, svnet_xyzblock_tier), the case table of tests/block_envelope_cases.py against them,
the Python admission rule against the C one, the tile kernels' division by multiplication, and the oracle's own conditioning on every case
(so that a failure of tests/test_hip_block_envelope.py means the kernel)."""
import itertools
import json
import os

import pytest
import torch

from tests import block_envelope_cases as T
from tests.common import case_errors
from tests.test_hip_train_parity import OUT        # the report directory of the existing block test: these reports go beside its


@pytest.fixture(scope="module")
def L():
    from svnet_amd import _lib
    return _lib.lib()


def _fused(case):
    return case[6] is not None


def _case_tiers(L, case):
    tag, (Cs, Cv), (Os, Ov), B, N, k, _ = case
    return {"fwd": L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N), "bwd": L.svnet_edgeblock_bwd_tier(Cs, Cv, Os),
            "wgrad": L.svnet_edgeblock_wgrad_tier(B * N * k, k, Os, T.used_tiles(Cs, Cv))}


def test_every_case_reaches_the_instantiation_the_table_states(L):
    from svnet_amd.models.sv_layers import edge_block_shape_ok, xyz_block_shape_ok
    for case in T.EDGE_CASES:
        tag, (Cs, Cv), (Os, Ov), B, N, k, expect = case
        assert edge_block_shape_ok(Cs, Cv, Os, Ov, k, N) == _fused(case), tag
        if _fused(case):
            assert _case_tiers(L, case) == expect, tag
    for tag, nc, (Os, Ov), B, N, k, tier in T.XYZ_CASES:
        assert xyz_block_shape_ok(Os, Ov, k) and L.svnet_xyzblock_tier(Os, Ov, nc) == tier, tag


def test_the_case_table_reaches_every_instantiation_of_the_envelope(L):
    """Every value the four tier functions return over the admitted envelope (all Cs 1..64, Cv 1..32, the five Os, Ov in {1, 32, 33, 64},
    k 2..64 at a few E) is reached by a case of the table: a tier added later without a case fails here."""
    Os_all, Ov_all = (8, 16, 32, 64, 128), (1, 32, 33, 64)
    fwd, bwd, wgrad, xyz = set(), set(), set(), set()
    for Cs, Cv, Os in itertools.product(range(1, 65), range(1, 33), Os_all):
        bwd.add(L.svnet_edgeblock_bwd_tier(Cs, Cv, Os))
        for Ov in Ov_all:
            fwd.add(L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, 2, 64))
        fwd.add(L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, 32, 8192, 8192))           # (B*N*6*Ov >= 2^30: no two-edge kernel)
        for k, points in itertools.product(range(2, 65), (1, 32, 33, 8192)):
            if (Cs, Cv) in ((32, 10), (64, 21), (64, 32), (1, 1)):                    # (the column-tile masks there are: 0x155, 0x3FF, 0x3FF, 0x155)
                wgrad.add(L.svnet_edgeblock_wgrad_tier(points * k, k, Os, T.used_tiles(Cs, Cv)))
    for Os, Ov, nc in itertools.product(range(1, 65), range(1, 65), (0, 2, 3)):
        xyz.add(L.svnet_xyzblock_tier(Os, Ov, nc))
    assert -1 not in fwd | bwd | xyz                                               # the enumeration stays inside the envelope
    fused = [c for c in T.EDGE_CASES if _fused(c)]
    reached = {key: {c[6][key] for c in fused} for key in ("fwd", "bwd", "wgrad")}
    reached["xyz"] = {c[6] for c in T.XYZ_CASES}
    found = {"fwd": fwd, "bwd": bwd, "wgrad": wgrad, "xyz": xyz}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "block_envelope_tiers.json"), "w") as f:
        json.dump({key: {"tiers": sorted(found[key]), "reached": sorted(reached[key])} for key in found}, f, indent=0)
    for key in found:
        assert found[key] == reached[key], "%s tiers %r, reached by the case table %r" % (key, sorted(found[key]), sorted(reached[key]))
    # what the enumeration must have found: 5 forward kernels, 3 x 5 tile kernels, the two affine GEMMs + "not served", 2 x 2 first-layer kernels
    assert len(fwd) == 5 and len(bwd) == 15 and wgrad == {-1, 1, 2} and xyz == {21, 22, 31, 32}


def test_python_admission_agrees_with_the_c_entry_points(L):
    """SVBlock._can_fuse's shape rule (edge_block_shape_ok) admits a shape exactly when the forward AND the backward entry point do
    (their SVNET_REQUIRE envelopes are the tier functions' -1), over the envelope and one step past each of its edges; the same for the
    first layer."""
    from svnet_amd.models.sv_layers import edge_block_shape_ok, xyz_block_shape_ok
    for Cs, Cv, Os, Ov in itertools.product(range(0, 67), range(0, 35), tuple(range(0, 137, 4)) + (7, 9, 127, 129, 256), (0, 1, 32, 33, 64, 65)):
        c_ok = L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, 2, 64) >= 0 and L.svnet_edgeblock_bwd_tier(Cs, Cv, Os) >= 0
        assert edge_block_shape_ok(Cs, Cv, Os, Ov, 20, 1024) == c_ok, (Cs, Cv, Os, Ov)
    for k, N in itertools.product((0, 1, 2, 7, 8, 64, 65), (1, 64, 8192, 8193)):
        assert edge_block_shape_ok(32, 10, 32, 10, k, N) == (2 <= k <= 64 and N <= 8192), (k, N)
        # the affine weight-gradient GEMM serves a subset of the admitted k: below 8 the block takes the dn_out + ternary GEMM path
        assert (L.svnet_edgeblock_wgrad_tier(2 * N * k, k, 32, 0x155) >= 0) == (8 <= k <= 64), (k, N)
    for Os, Ov, nc in itertools.product(range(0, 67), range(0, 67), (0, 1, 2, 3, 4)):
        assert (L.svnet_xyzblock_tier(Os, Ov, nc) >= 0) == (xyz_block_shape_ok(Os, Ov, 20) and nc in (0, 2, 3)), (Os, Ov, nc)
    assert not xyz_block_shape_ok(32, 10, 65) and xyz_block_shape_ok(32, 10, 64)


def test_small_div_is_exact_for_every_row_offset_the_kernels_form():
    """n / k as (n * ceil(65536 / k)) >> 16 (small_div of csrc/edgeblock_bwd.hip, the kmagic cursors of csrc/gemm_mfma.hip).  The largest n a
    kernel forms: the tile kernel divides t0 + off with t0 < k <= 64 (slot of the tile's first row) and off < 64 (cursor_init: off < TE = 32;
    phase C: 8 * wave + lane / 8 < 40), so n <= 126; mfma_tn_tern divides cur_t + 8 h (h < 2) and cur_t + 16 with cur_t < k, so n <= 79;
    mfma_tn_aff2 divides cur_t + 32, n <= 95.  Checked for every n < 1024 - what small_div's comment promises - in 32-bit arithmetic."""
    for k in range(2, 65):
        kmagic = (65536 + k - 1) // k
        n = torch.arange(0, 1024, dtype=torch.int64)
        assert int((n * kmagic).max()) < 1 << 32                      # the product fits the kernels' uint32
        assert torch.equal((n * kmagic) >> 16, n // k), k


def _worst(errs):
    return max(errs.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("case", T.EDGE_CASES, ids=[c[0] for c in T.EDGE_CASES])
def test_edge_oracle_is_well_conditioned(case):
    """The fp32 oracle against the float64 oracle on one graph: every output, gradient and running statistic within 1e-4 - the inputs
    leave a kernel test ten times that before rounding is a suspect."""
    inputs = T.edge_inputs(case)
    idx = T.edge_oracle_graph(case, inputs)
    r32, r64 = T.edge_oracle(case, inputs, idx, torch.float32), T.edge_oracle(case, inputs, idx, torch.float64)
    errs = case_errors(r32, r64)
    print("oracle fp32 vs float64 (%s): worst %.3e on %s, outputs %.3e" % (case[0], *_worst(errs)[::-1], max(errs["out0"], errs["out1"])))
    assert set(errs) == set(r64) and _worst(errs)[1] <= T.OUT_RTOL, sorted(errs.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize("case", T.XYZ_CASES, ids=[c[0] for c in T.XYZ_CASES])
def test_first_layer_oracle_is_well_conditioned(case):
    from oracle import sv_ref
    inputs = T.xyz_inputs(case)
    idx = sv_ref.knn_indices(inputs[1], case[5])
    r32, r64 = T.xyz_oracle(case, inputs, idx, torch.float32), T.xyz_oracle(case, inputs, idx, torch.float64)
    errs = case_errors(r32, r64)
    print("oracle fp32 vs float64 (%s): worst %.3e on %s, outputs %.3e" % (case[0], *_worst(errs)[::-1], max(errs["out0"], errs["out1"])))
    assert set(errs) == set(r64) and _worst(errs)[1] <= T.OUT_RTOL, sorted(errs.items(), key=lambda kv: -kv[1])[:4]
