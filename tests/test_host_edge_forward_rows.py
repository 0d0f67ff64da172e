"""CPU tests (no GPU, nothing allocated) of the bound behind the forward edge kernels' 32-bit neighbour rows (csrc/edgeblock.hip
edge_rows_fit_32): the kernels address a neighbour's row by a 32-bit BYTE offset into the point tables s [B N Cs], v [B N 3 Cv],
ut [B N 6 Ov] and zz [B N 18], so the widest of them must stay below 2^30 floats.  svnet_edgeblock_fwd_tier states the bound for the
two-edge kernel, which has no 64-bit form: on the far side it returns the one-edge tier, whose launch then takes the 64-bit instantiation.
The one-edge tiers themselves do not depend on B and N.  Also here: what tests/test_hip_edge_forward_masks.py says about k = 1."""
import pytest


@pytest.fixture(scope="module")
def L():
    from svnet_amd import _lib
    return _lib.lib()


def _widest(Cs, Cv, Ov):
    return max(Cs, 3 * Cv, 6 * Ov, 18)


# (Cs, Cv, Os, Ov), all served by the two-edge kernel at small sizes; the widest table is ut, ut, s, zz, v
TWO_EDGE_SHAPES = [(32, 10, 32, 10), (32, 16, 32, 32), (32, 1, 8, 1), (1, 1, 8, 1), (8, 16, 16, 2)]


@pytest.mark.parametrize("shape", TWO_EDGE_SHAPES, ids=["%d_%d_%d_%d" % s for s in TWO_EDGE_SHAPES])
def test_two_edge_kernel_is_chosen_exactly_below_the_32_bit_bound(L, shape):
    from svnet_amd._lib import DEFINES
    Cs, Cv, Os, Ov = shape
    two, one_edge = DEFINES["SVNET_EDGE_FWD_TWO"], 111
    last = ((1 << 30) - 1) // _widest(Cs, Cv, Ov)              # the largest B*N whose widest table has fewer than 2^30 floats
    assert last * _widest(Cs, Cv, Ov) < 1 << 30 <= (last + 1) * _widest(Cs, Cv, Ov)
    for B, N in ((1, last), (last, 1)):
        assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N) == two, (B, N)
    for B, N in ((1, last + 1), (last + 1, 1), (2, last // 2 + 1)):
        assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N) == one_edge, (B, N)
    # the model's sizes, and sizes whose product does not fit 64 bits (no wrap-around back into the bound)
    assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, 32, 1024) == two
    assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, 1 << 40, 1 << 40) == one_edge
    assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, 3, (1 << 63) - 1) == one_edge


def test_the_bound_is_the_widest_table_not_only_ut(L):
    """Cs = 32 against Ov = 1: s rows are 32 floats, ut rows 6.  B*N = 2^25 fills s to 2^30 floats while ut holds 6 * 2^25 < 2^30."""
    from svnet_amd._lib import DEFINES
    assert L.svnet_edgeblock_fwd_tier(32, 1, 8, 1, 1 << 12, (1 << 13) - 1) == DEFINES["SVNET_EDGE_FWD_TWO"]
    assert L.svnet_edgeblock_fwd_tier(32, 1, 8, 1, 1 << 12, 1 << 13) == 111


def test_one_edge_tiers_do_not_depend_on_the_size(L):
    for (Cs, Cv, Os, Ov), tier in (((32, 10, 64, 21), 111), ((64, 21, 64, 21), 110), ((32, 10, 128, 42), 121), ((64, 21, 128, 42), 120)):
        for B, N in ((2, 24), (32, 1024), (8192, 8192), (1 << 20, 1 << 20)):
            assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N) == tier, (Cs, Cv, Os, Ov, B, N)


def test_the_fused_path_admits_no_k1(L):
    from svnet_amd.models.sv_layers import edge_block_shape_ok
    from tests import block_envelope_cases as T
    from tests.test_hip_edge_forward_masks import B, CASES, N
    for _, (Cs, Cv), (Os, Ov), k, tier in CASES:
        assert edge_block_shape_ok(Cs, Cv, Os, Ov, k, N) and not edge_block_shape_ok(Cs, Cv, Os, Ov, 1, N)
        assert L.svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N) == tier and L.svnet_edgeblock_bwd_tier(Cs, Cv, Os) >= 0
        assert L.svnet_edgeblock_wgrad_tier(B * N, 1, Os, T.used_tiles(Cs, Cv)) == -1


def test_the_oracle_is_well_conditioned_on_the_forward_mask_cases():
    """fp32 against float64 oracle on one graph, as tests/test_host_block_envelope.py does for its table: within 1e-4 on every key, so
    that a failure of tests/test_hip_edge_forward_masks.py means the kernel and not a sign decision on a knife edge of rounding."""
    import torch
    from tests import block_envelope_cases as T
    from tests.common import case_errors
    from tests.test_hip_edge_forward_masks import CASES, _ecase
    for case in CASES:
        ecase = _ecase(case)
        inputs = T.edge_inputs(ecase)
        idx = T.edge_oracle_graph(ecase, inputs)
        r32, r64 = T.edge_oracle(ecase, inputs, idx, torch.float32), T.edge_oracle(ecase, inputs, idx, torch.float64)
        errs = case_errors(r32, r64)
        # (Ov = 1 leaves the gate MLP a hidden layer of width 0: its weights are empty arrays, which case_errors passes over)
        assert set(errs) == {n for n in r64 if r64[n].size} and max(errs.values()) <= T.OUT_RTOL, (case[0], sorted(errs.items(), key=lambda kv: -kv[1])[:4])
