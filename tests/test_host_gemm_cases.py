"""CPU tests of svnet_gemm_f32's dispatch and of the comparison the GPU test applies (tests/gemm_cases.py).

The queries svnet_gemm_tier / svnet_gemm_variant are pure host functions: they run here on descriptors of fake, non-null addresses with
each case's real alignments (nothing is dereferenced or launched).  The second half checks the yardstick itself: that the int cases stay
exact in float32, that plain float32 references sit well inside the bound of the real cases, and that the comparison has teeth - a
reference that lost one term of one element, or the third bf16 piece of an operand, is rejected."""
import ctypes

import numpy as np
import pytest

from svnet_amd import _lib
from tests import gemm_cases as G

IDS = [c["name"] for c in G.CASES]
NONEMPTY = [c for c in G.RUN_CASES if c["M"] and c["N"] and c["K"]]


def _query(c):
    L = _lib.lib()
    d = G.fill_desc(c, G.fake_pointers(c))
    return L.svnet_gemm_tier(ctypes.byref(d)), L.svnet_gemm_variant(ctypes.byref(d))


@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c["name"] for c in G.RUN_CASES])
def test_case_reaches_the_family_and_variant_it_names(c):
    tier, variant = _query(c)
    assert (G.FAMILY.get(tier, tier), variant) == (G.FAMILY[c["tier"]], c["variant"]), c["name"]


@pytest.mark.parametrize("c", G.REFUSALS, ids=[c["name"] for c in G.REFUSALS])
def test_refusals_return_their_codes(c):
    assert _query(c) == (c["rc"], c["rc"])
    assert _lib.lib().svnet_last_error()                                        # and say why


def test_null_descriptor_and_null_operands_are_argument_errors():
    L = _lib.lib()
    assert L.svnet_gemm_tier(None) == G.E_ARG and L.svnet_gemm_variant(None) == G.E_ARG
    c = G.by_name("t_64x64x16")
    for field in ("A", "B", "C"):
        d = G.fill_desc(c, G.fake_pointers(c))
        setattr(d, field, None)
        assert L.svnet_gemm_tier(ctypes.byref(d)) == G.E_ARG, field
    d = G.fill_desc(c, G.fake_pointers(c))
    d.c_cs = 0
    assert L.svnet_gemm_tier(ctypes.byref(d)) == G.E_ARG
    d = G.fill_desc(c, G.fake_pointers(c))
    d.M = -1
    assert L.svnet_gemm_tier(ctypes.byref(d)) == G.E_ARG


def test_every_family_and_variant_is_named_by_a_case():
    by = {}
    for c in G.RUN_CASES:
        by.setdefault(c["tier"], set()).add(c["variant"])
    assert set(by) == set(G.FAMILY)
    rows = by[G.ROWS]
    assert {v & 15 for v in rows} == {1, 2, 4, 8}                               # NT
    assert {v >> 4 & 1 for v in rows} == {0, 1} and {v >> 5 & 1 for v in rows} == {0, 1} and {v >> 6 & 1 for v in rows} == {0, 1}
    assert {(v >> 4 & 1, v >> 5 & 1) for v in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}     # mfma_rows_kernel<., AVEC, DEEP>
    assert by[G.ROWS_LDS] == {0, 1}
    assert {v & 15 for v in by[G.ROWS_SPLIT]} == {1, 2, 4} and {v >> 4 for v in by[G.ROWS_SPLIT]} == {4, 2, 1}
    assert by[G.TN_FP32] == {G.v_tn(2, 2), G.v_tn(2, 1), G.v_tn(1, 2), G.v_tn(1, 1)}
    tern = by[G.TN_TERN]
    assert {v & 15 for v in tern} == {1, 2, 4, 5} and {v >> 4 & 15 for v in tern} == {1, 2, 4}
    assert {v >> 8 & 1 for v in tern} == {0, 1} and {v >> 9 & 1 for v in tern} == {0, 1}
    assert by[G.DOT] == {0}
    assert 1 in by[G.TILE] and {2, 3, 5} <= by[G.TILE]


@pytest.mark.parametrize("below,above", G.BOUNDARY_PAIRS, ids=["%s|%s" % p for p in G.BOUNDARY_PAIRS])
def test_boundary_pairs_fall_on_their_two_sides(below, above):
    lo, hi = G.by_name(below), G.by_name(above)
    assert _query(lo) == (lo["tier"], lo["variant"]) and _query(hi) == (hi["tier"], hi["variant"])
    assert (lo["tier"], lo["variant"]) != (hi["tier"], hi["variant"])


def test_the_named_boundaries_differ_in_one_quantity_only():
    """M = 15 / 16, K = 7 / 8, K = 1023 / 1024, M N = 8192 / 8193, M = 4095 / 4096 (workspace), M = 1023 / 1024 (3x workspace)."""
    def shape(n):
        c = G.by_name(n)
        return c["M"], c["N"], c["K"]
    assert shape("t_exact_m15") == (15, 20, 16) and shape("r_m16") == (16, 20, 16)
    assert shape("t_exact_k7")[2] == 7 and shape("r_k8")[2] == 8 and shape("t_exact_k7")[:2] == shape("r_k8")[:2]
    assert shape("t_tn_k1023") == (100, 100, 1023) and shape("n_k1024") == (100, 100, 1024)
    assert np.prod(shape("d_mn8192")[:2]) == 8192 and np.prod(shape("t_mn8193")[:2]) == 8193
    assert shape("r_packed_m4095") == (4095, 257, 68) and shape("l_m4096") == (4096, 257, 68)
    assert shape("t_split_m1023") == (1023, 64, 16) and shape("s_n64") == (1024, 64, 16)
    for a, b in (("r_packed_m4095", "l_m4096"), ("t_split_m1023", "s_n64")):
        assert G.by_name(a)["ws"] == G.by_name(b)["ws"] > 0


def _drop_one_term(c, x, r):
    """The expected storage with one non-zero term of one live, unmasked element missing (searched from the last element)."""
    A = np.asarray(x.A, dtype=np.float64) if c["M"] * c["K"] <= 1 << 22 else None
    live = G.live_rows(c) if c["tern"] else np.ones(c["M"], bool)
    cs = 1.0 if x.col_scale is None else x.col_scale.astype(np.float64)
    for i in range(c["M"] - 1, -1, -1):
        if not live[i]:
            continue
        a = (A[i] if A is not None else np.asarray(x.A[i], dtype=np.float64)) * (1.0 if x.a_scale is None else x.a_scale)
        terms = a[:, None] * np.asarray(x.B, dtype=np.float64) * (x.alpha * cs)            # [K, N]
        if x.mask is not None:
            terms = terms * x.mask_bits[i][None, :]
        k, j = np.unravel_index(int(np.abs(terms).argmax()), terms.shape)
        if terms[k, j] != 0:
            bad = G.Ref()
            bad.C = r.C.copy()
            bad.C[i, j] -= terms[k, j]
            return G.expected_store(c, x, bad), (i, j, k), terms[k, j]
    raise AssertionError("%s: no non-zero term to drop" % c["name"])


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c["name"] for c in G.RUN_CASES])
def test_the_comparison_on_every_case(c, kind):
    x = G.build(c, kind)
    r = G.reference(c, x)
    # the reference itself passes, gaps and all
    good = G.expected_store(c, x, r)
    assert G.failures(c, x, r, good, r.col_sum) == []
    if kind == "int":
        # exact in float32 whatever the order: every sum of magnitudes, and every column sum of them, stays below 2^24
        assert r.mag.size == 0 or r.mag.max() < 2 ** 24, r.mag.max()
        if r.col_sum is not None:
            assert r.col_mag.max() < 2 ** 24, r.col_mag.max()
        assert np.array_equal(r.C.astype(np.float32).astype(np.float64), r.C)
    elif r.C.size:
        # float32 references stay within a quarter of the bound
        for which, (v, col) in zip(("matmul", "sequential"), G.refs_f32(c, x)):
            worst, at, cw = G.ratios(c, x, r, v, col)
            assert max(worst, cw) <= G.C_BOUND / 4, (c["name"], which, worst, at, cw)
    if c in NONEMPTY:
        # one term dropped from one element
        bad, where, term = _drop_one_term(c, x, r)
        assert G.failures(c, x, r, bad, r.col_sum), (c["name"], kind, where)
        if r.col_sum is not None and kind == "int":     # (one term of a real column sum over 2^18 rows is below that sum's own bound)
            col = r.col_sum.copy()
            col[where[1]] -= term
            assert G.failures(c, x, r, good, col), (c["name"], kind, "col_sum", where)
        # a written gap
        if (~x.written).any():
            gap = good.copy()
            gap[np.flatnonzero(~x.written)[-1]] = 0.0
            assert G.failures(c, x, r, gap, r.col_sum), (c["name"], kind, "gap")
        # the fp32 operand of a bf16-split family cut to 16 significant bits (the third piece lost)
        if kind == "real" and c["tier"] in G.SPLIT_FAMILIES:
            lost = G.reference(c, x, B=G.truncated(x.B)) if c["tern"] else G.reference(c, x, A=G.truncated(x.A))
            assert G.failures(c, x, r, G.expected_store(c, x, lost), r.col_sum), (c["name"], "truncated operand passes")
