"""CPU tests of the vector tail's case table (no GPU): tests/vtail_cases.py's restated plan against what the library reports, and the
reference alone on every case - float32 against float64 within a quarter of the GPU tests' bounds, the float32 arg-max replayed into the
float64 run within Decisions.check()'s cap - so that a failure of test_hip_kernel_tiers.py's vector-tail section means the kernel."""
import numpy as np
import pytest
import torch

from tests import vtail_cases as T
from tests.common import case_errors

IDS = [c[0] for c in T.CASES]


def test_restated_plan_is_the_librarys_and_the_table_states_it():
    """svnet_vtail_workspace_bytes(B, N, C) = 3 B C * (8 + 4 * chunks): the chunk count read from the library equals the restated plan's,
    and every figure the table states about a case is what the restated plan gives."""
    from svnet_amd import _lib
    L = _lib.lib()
    for tag, B, N, C, expect in T.CASES:
        assert T.plan_of(B, N, C) == expect, (tag, T.plan_of(B, N, C))
        nb = L.svnet_vtail_workspace_bytes(B, N, C)
        assert nb % (3 * B * C) == 0 and (nb // (3 * B * C) - 8) % 4 == 0, (tag, nb)
        assert (nb // (3 * B * C) - 8) // 4 == expect[2], (tag, nb, expect)
    # the restated rule beyond the table: a sweep of shapes around the row multiples and the target
    for B in (1, 2, 3, 95, 96, 97, 767, 768, 769, 65535):
        for N in (256, 257, 263, 264, 265, 1000, 1024, 4099):
            chunks = T.vtail_plan(B, N)[1]
            assert L.svnet_vtail_workspace_bytes(B, N, 7) == 3 * B * 7 * (8 + 4 * chunks), (B, N)
    # the edges the table is there to reach
    got = {c[0]: c[4] for c in T.CASES}
    assert {e[0] for e in got.values()} == {1, 2, 3} and sorted(c[3] for c in T.CASES if c[3] in (1, 64, 65, 128, 129, 192)) == [1, 64, 65, 128, 129, 192]
    assert {got["c64_last_of_1"][4], got["c129_last_of_3"][4], got["c65_last_of_5"][4]} == {1, 3, 5}
    assert got["one_chunk"][2] == 1 and got["chunk_removed"][1] - got["chunk_removed"][2] == 1


def test_cases_are_admitted_and_their_neighbours_refused():
    """The admission rule of _ops.GlobalMaxMeanPoolBNV.supported in library terms: the scalar half needs a split path (N >= 256,
    B <= 65535), the vector half C <= 192."""
    from svnet_amd import _lib
    L = _lib.lib()
    for tag, B, N, C, _ in T.CASES:
        assert C <= 192 and L.svnet_pool_workspace_bytes(B, N, T.CA, 0) > 0 and L.svnet_pool_workspace_bytes(B, N, T.CA, 1) > 0, tag
    assert L.svnet_pool_workspace_bytes(2, 255, T.CA, 0) == 0


def _report(tag, errs, b):
    k, e = max(errs.items(), key=lambda kv: kv[1] / b[kv[0]])
    print("vtail oracle fp32 vs float64 (%s): worst %.3e of %.1e on %s" % (tag, e, b[k], k))


def _conditioned(r32, r64, dec, name):
    summary = dec.check()                                     # no more forced arg-max than the cap, none uncertified
    errs, b = case_errors(r32, r64), T.bounds(r64)
    _report(name, errs, b)
    assert set(errs) == set(r64)
    for k, e in errs.items():
        assert e <= T.CONDITION * b[k], "%s/%s: the float32 reference is %.3e from float64, bound %.1e" % (name, k, e, b[k])
    return summary


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("tag", IDS)
def test_reference_is_well_conditioned_and_its_argmax_within_the_cap(tag, train):
    r32, r64, dec, _, _ = T.conditioning(tag, train)
    assert set(r64) == set(T.KEYS) and next(iter(r64)) == "out"
    _conditioned(r32, r64, dec, "%s %s" % (tag, "train" if train else "eval"))


@pytest.mark.parametrize("tag", ["c64_last_of_1", "c129_last_of_3"])
@pytest.mark.parametrize("form", ["no_gate", "fp_weight"])
def test_optional_operand_forms_are_well_conditioned(form, tag):
    r32, r64, dec, _, _ = T.conditioning(tag, True, None, form != "no_gate", form != "fp_weight")
    assert ("dgate" in r64) == (form != "no_gate") and ("d:scz" in r64) == (form != "fp_weight")
    _conditioned(r32, r64, dec, "%s %s" % (tag, form))


def test_zero_vector_case_is_well_conditioned_in_both_parts_of_dv():
    """The reference's dv at the zero vectors is ~1e6 times an ordinary entry; each part holds the quarter bound against its own maximum."""
    inp = T.inputs(T.BY_TAG["c65_last_of_5"], "zeros")
    zero = T.zero_vectors(inp["v"]).numpy()
    assert 0 < zero.sum() < 0.01 * zero.size and zero[1, 256, :, 2].all() and zero[1, 260, :, 64].all()
    r32, r64, dec, _, _ = T.conditioning("c65_last_of_5", True, "zeros")
    big, rest = np.abs(r64["dv"][zero]).max(), np.abs(r64["dv"][~zero]).max()
    print("vtail zero vectors: largest |dv| %.3e at the zero vectors, %.3e elsewhere" % (big, rest))
    assert big > 1e3 * rest                                    # what makes one bound over the whole tensor empty
    assert not np.abs(r64["dv"][zero]).min() == 0.0            # (the gradient THROUGH a zero vector's scale is not zero; the norm's is)
    for part32, part64 in zip(T.split_dv(r32, zero), T.split_dv(r64, zero)):
        e = case_errors(part32, part64)["dv"]
        assert e <= T.CONDITION * T.GRAD_RTOL, e
    rest32, rest64 = ({k: v for k, v in r.items() if k != "dv"} for r in (r32, r64))
    _conditioned(rest32, rest64, dec, "c65_last_of_5 zeros")


def test_tie_case_gives_the_copies_enough_columns():
    """The three copies of one point (rows 31, 32, 256; scaled by 4) hold the float64 maximum of at least 3C / 4 vector columns over the
    batch, and the float32 reference's values at the copies are the same bits - the tie is exact, the first row must take it."""
    tag, B, N, C, _ = T.BY_TAG["c64_last_of_1"]
    r32, r64, dec, arg32, f64 = T.conditioning(tag, True, "ties")
    own = f64.argmax(dim=1)[:, T.CA:]
    at_copy = sum(own == r for r in T.TIE_ROWS).bool()
    print("vtail ties: the copies hold the maximum of %d of %d vector columns" % (int(at_copy.sum()), at_copy.numel()))
    assert int(at_copy.sum()) >= 3 * C // 4
    assert bool((arg32[:, T.CA:][at_copy] == T.TIE_ROWS[0]).all())          # torch.max: the first index of an exact tie
    _conditioned(r32, r64, dec, "c64_last_of_1 ties")


def test_replay_of_a_far_row_is_refused():
    """The teeth of the replay on the CPU: one arg-max moved to the row of the column's smallest value fails Decisions.check()."""
    tag = "c65_last_of_5"
    _, _, _, arg32, f64 = T.conditioning(tag, True)
    bad = arg32.clone()
    bad[1, T.CA + 7] = int(f64[1, :, T.CA + 7].argmin())
    _, info = T.reference(T.inputs(T.BY_TAG[tag]), torch.float64, True, pools=bad)
    with pytest.raises(AssertionError, match="decision replay"):
        info["dec"].check()
