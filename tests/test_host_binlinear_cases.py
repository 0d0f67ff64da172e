"""CPU tests of the binarized dense layer's dispatch and of the comparison the GPU test applies (tests/binlinear_cases.py).

svnet_binlinear_tier / svnet_binlinear_i8_tier are pure host functions of the sizes: they run here, and every case must reach the tier
it names.  The refusals that the entry points decide before any launch are called with fake, non-null addresses (nothing is
dereferenced: every one of them returns before the first launch, and all but the rows_per_cloud check with M = 0, which would launch
nothing anyway).  The second half checks the yardstick: the restatement's plane layout against tests/decisions.py, the exact kind's
claim to be exact, and that the comparators have teeth."""
import numpy as np
import pytest
import torch

from svnet_amd import _lib
from tests import binlinear_cases as B
from tests import binlinear_ref as R
from tests.decisions import decode_rows

FAKE = [0x7F0000000000 + 0x10000000 * i for i in range(16)]


@pytest.mark.parametrize("c", B.POPCOUNT, ids=[c["name"] for c in B.POPCOUNT])
def test_popcount_case_reaches_the_tier_it_names(c):
    for chunk in range(len(c["chunks"])):
        rc, got = B.plan_of(c, chunk)
        want = B.expected_plan(c, chunk)
        assert rc == 0 and got == want, (c["name"], chunk, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    assert B.plan_of(c, len(c["chunks"]))[0] == B.E_ARG                           # no chunk past the last


@pytest.mark.parametrize("c", B.I8, ids=[c["name"] for c in B.I8])
def test_i8_case_reaches_the_tier_it_names(c):
    rc, got = B.i8_plan_of(c)
    assert rc == 0 and got == B.expected_i8_plan(c), (c["name"], got)
    assert not c["cloud"] or c["M"] % c["cloud"] == 0


def test_every_tier_is_named_by_a_case():
    tiers = {(kwm, c["ppm"], c["form"][0]) for c in B.POPCOUNT for _, kwm in c["chunks"]}
    assert tiers == {(kwm, 1, f) for kwm in (2, 4, 8, 16, 34) for f in (B.TILE_SPLIT, B.GROUPS, B.LOOP)} | {(kwm, 2, B.LOOP) for kwm in (2, 4, 8)}
    assert {len(c["chunks"]) for c in B.POPCOUNT} == {1, 2, 3}
    for n in (2, 3):                                                              # chunked K in all three forms, with and without planes
        assert {(c["form"][0], c["planes"]) for c in B.POPCOUNT if len(c["chunks"]) == n} == {(f, p) for f in B.FORM for p in (0, 1)}
    loops = [c for c in B.POPCOUNT if c["form"][0] == B.LOOP]
    assert {c["form"][1] for c in loops} == {5, 6, 7, 8}
    wide = {(c["form"][0], c["form"][1] < 8) for c in B.POPCOUNT if c["chunks"][0][1] == 34 and len(c["chunks"]) == 1}
    assert wide == {(B.TILE_SPLIT, True), (B.GROUPS, False), (B.LOOP, True), (B.LOOP, False)}
    assert any(c["form"][3] == 2 for c in loops) and any(c["M"] > 64 * c["form"][4] for c in loops)      # two launches; a second tile pass
    assert {kwm for c in B.POPCOUNT if c["ldx_pad"] for _, kwm in c["chunks"]} == {2, 4, 8, 16, 34}
    assert any(c["O"] == 1 for c in B.POPCOUNT) and any(not c["bias"] for c in B.POPCOUNT)
    assert {c["K"] for c in B.POPCOUNT} >= {1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2176, 2177, 2240, 4353}
    big = {(c["K"], c["O"]) for c in B.POPCOUNT_DEVICE}
    assert big == {(3, 257), (130, 257), (300, 257), (513, 257), (3, 5)} and all(c["M"] == 131073 for c in B.POPCOUNT_DEVICE)

    assert {(c["ntw"], c["grid_y"]) for c in B.I8} >= {(1, 1), (2, 1), (4, 1), (4, 2)}
    assert {(c["ntw"], c["planes"], c["sums"], bool(c["cloud"])) for c in B.I8} == {(n, p, s, k) for n in (1, 2, 4) for p in (0, 1) for s in (0, 1)
                                                                                    for k in (False, True)}
    assert {c["M"] for c in B.I8} >= {1, 8, 63, 64, 65, 127, 128, 129, 200, 257}
    assert {c["K"] for c in B.I8} == {1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300}
    assert {c["O"] for c in B.I8} == {1, 31, 32, 33, 128, 129, 256, 257, 512, 513, 1025}
    assert {c["cloud"] for c in B.I8 if c["cloud"] and c["cloud"] != c["M"]} >= {1, 7, 128, 300} and any(c["cloud"] == c["M"] for c in B.I8)
    assert {c["bias"] for c in B.I8} == {0, 1} and {c["ldx_pad"] for c in B.I8} == {0, 5}

    assert {(c["O"], c["K"]) for c in B.PREPARE} == {(1, 1), (3, 63), (5, 64), (7, 65), (40, 130)}
    assert {(c["O"], c["K"]) for c in B.GRAD} == {(1, 1), (3, 63), (5, 65), (40, 130), (5000, 3)}
    for field, values in (("accumulate", {0, 1}), ("eval", {0, 1}), ("gx_sliced", {0, 1}), ("sum_len", {0, 1, 65})):
        assert {c[field] for c in B.GRAD} == values


def test_refusals_decided_before_any_launch_return_their_codes():
    L = _lib.lib()
    plan, plan8 = _lib.STRUCTS["svnet_binlinear_plan"](), _lib.STRUCTS["svnet_binlinear_i8_plan"]()
    x, beta, ws, wz, sc, bs, y, p0, p1, p2, sums, cn = FAKE[:12]

    def fwd(M=0, K=70, O=40, ldx=None, ptrs=None, planes=(None, None, None)):
        a = dict(x=x, beta=beta, ws=ws, wz=wz, sc=sc, y=y)
        a.update(ptrs or {})
        return L.svnet_binlinear_fwd_f32(a["x"], K if ldx is None else ldx, a["beta"], a["ws"], a["wz"], a["sc"], bs, M, K, O, a["y"], *planes, None)

    def fwd8(M=0, K=70, O=40, ldx=None, ptrs=None, planes=(None, None, None), col=None, cloud=None):
        a = dict(x=x, beta=beta, w8=ws, sc=sc, y=y)
        a.update(ptrs or {})
        args = (a["x"], K if ldx is None else ldx, a["beta"], a["w8"], a["sc"], bs, M, K, O, a["y"], *planes, col)
        if cloud is None:
            return L.svnet_binlinear_i8_fwd_f32(*args, None)
        return L.svnet_binlinear_i8_cloud_fwd_f32(*args, cloud[0], cloud[1], None)

    assert fwd() == 0 and fwd8() == 0 and fwd8(cloud=(cn, 1)) == 0                 # (M = 0: valid, and nothing to launch)
    # K or O over the limits: the query and the entry point alike
    for K, O in ((1 << 20) + 1, 40), (70, (1 << 20) + 1):
        assert L.svnet_binlinear_tier(5, K, O, 0, plan) == B.E_UNSUPPORTED and fwd(K=K, O=O) == B.E_UNSUPPORTED
    assert L.svnet_binlinear_tier(5, 1 << 20, 1 << 20, 0, plan) == 0
    for K, O in (1 << 24, 40), (70, 1 << 24):
        assert L.svnet_binlinear_i8_tier(5, K, O, 0, plan8) == B.E_UNSUPPORTED and fwd8(K=K, O=O) == B.E_UNSUPPORTED
    # column sums square the count in int32: K <= 46340
    assert L.svnet_binlinear_i8_tier(5, 46340, 40, 1, plan8) == 0 and L.svnet_binlinear_i8_tier(5, 46341, 40, 0, plan8) == 0
    assert L.svnet_binlinear_i8_tier(5, 46341, 40, 1, plan8) == B.E_UNSUPPORTED
    assert fwd8(K=46341, col=sums) == B.E_UNSUPPORTED and fwd8(K=46341) == 0 and fwd8(K=46340, col=sums) == 0
    assert L.svnet_last_error()
    # bad sizes
    for M, K, O in ((-1, 70, 40), (5, 0, 40), (5, 70, 0)):
        assert L.svnet_binlinear_tier(M, K, O, 0, plan) == B.E_ARG and L.svnet_binlinear_i8_tier(M, K, O, 0, plan8) == B.E_ARG
        assert fwd(M=M, K=K, O=O) == B.E_ARG and fwd8(M=M, K=K, O=O) == B.E_ARG
    assert fwd(ldx=69) == B.E_ARG and fwd8(ldx=69) == B.E_ARG
    assert L.svnet_binlinear_tier(5, 70, 40, 1, plan) == B.E_ARG and L.svnet_binlinear_tier(5, 70, 40, -1, plan) == B.E_ARG
    assert L.svnet_binlinear_tier(5, 70, 40, 0, None) == B.E_ARG and L.svnet_binlinear_i8_tier(5, 70, 40, 0, None) == B.E_ARG
    # one or two of the three planes
    for planes in ((p0, None, None), (None, p1, None), (None, None, p2), (p0, p1, None), (p0, None, p2), (None, p1, p2)):
        assert fwd(planes=planes) == B.E_ARG and fwd8(planes=planes) == B.E_ARG
    assert fwd(planes=(p0, p1, p2)) == 0 and fwd8(planes=(p0, p1, p2)) == 0
    # rows_per_cloud must divide M; the cloud entry needs its counts
    assert fwd8(M=10, cloud=(cn, 3)) == B.E_ARG and fwd8(M=10, cloud=(cn, 0)) == B.E_ARG and fwd8(M=10, cloud=(cn, -5)) == B.E_ARG
    assert fwd8(cloud=(None, 1)) == B.E_ARG
    # null pointers
    for name in ("x", "beta", "ws", "wz", "sc", "y"):
        assert fwd(ptrs={name: None}) == B.E_ARG, name
    for name in ("x", "beta", "w8", "sc", "y"):
        assert fwd8(ptrs={name: None}) == B.E_ARG, name
    assert L.svnet_binweight_prepare_f32(None, None, 3, 3, None, None, None, None, None) == B.E_ARG
    assert L.svnet_binweight_prepare_f32(x, None, 3, 3, None, None, None, y, None) == B.E_ARG          # w_eff needs scale
    assert L.svnet_binweight_prepare_f32(x, None, 3, 3, ws, None, None, None, None) == B.E_ARG         # one plane of two
    assert L.svnet_binweight_grad_f32(None, x, sc, 3, 3, y, y, 0, 0, None, 0, None) == B.E_ARG
    assert L.svnet_binweight_grad_f32(x, x, sc, 3, 3, y, y, 0, 0, sums, 0, None) == B.E_ARG            # sum_buf without a length


SMALL = [c for c in B.POPCOUNT_HOST if c["M"] * c["K"] * c["O"] <= 3 * 10 ** 7] + B.I8


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_the_restatement_on_every_small_case(c):
    """The plane layout round-trips through tests/decisions.py, the exact kind is exact in float32, the reference passes its own
    comparison, and the planted boundary values are where they are meant to be."""
    M, K = c["M"], c["K"]
    for kind in B.KINDS:
        d = B.build_forward(c, kind)
        r = B.reference_forward(c, d)
        sign, ste = decode_rows(M, K, [torch.from_numpy(r[n].view(np.int64)) for n in ("x_sign", "x_nz", "x_ste")])
        t = r["t"]
        assert np.array_equal(sign.numpy(), np.sign(t)) and np.array_equal(ste.numpy() == 1, np.abs(t) <= B.F12)
        assert np.abs(r["count"] - (0 if d.cloud_n is None else np.repeat(d.cloud_n.astype(np.int64), c["cloud"], axis=0))).max() <= K
        if kind == "exact":
            assert B.exact_kind_is_exact(r)
        y = B.y_storage(c)
        y[:M] = r["y"].astype(np.float32)
        planes = {n: np.concatenate([r[n], np.full((1, K), B.PLANE_SENTINEL)]) for n in ("x_sign", "x_nz", "x_ste")}
        assert B.y_failures(c, kind, r, y) == [] and B.plane_failures(c, r, planes) == []
        if M * K >= 256:
            assert all(n > 0 for n in d.hits.values()), d.hits
            for v in (B.F12, -B.F12):
                assert np.any(t == v) and np.any(t == -v)
            assert np.any(t == B.F12_UP) and np.any(t == -B.F12_UP) and np.any(t == 0) and np.any(np.signbit(d.x) & (d.x == 0))
            assert np.any(d.W == 0) and np.any(np.abs(d.W) == B.F12) and np.any(np.abs(d.W) == B.F12_UP)


TEETH = [B.by_name(B.POPCOUNT, n) for n in ("k65_split", "k257_groups", "k1025_loop", "chunk2177_loop_og8")] + [B.by_name(B.I8, "n2_psc7_m63x3")]


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", TEETH, ids=[c["name"] for c in TEETH])
def test_the_comparators_have_teeth(c, kind):
    """A correct result is rejected against a reference with one weight sign flipped, one plane bit flipped, a count off by 2, or the STE
    threshold moved by one ulp; a written guard is rejected too."""
    M, K, O = c["M"], c["K"], c["O"]
    d = B.build_forward(c, kind)
    r = B.reference_forward(c, d)
    y = B.y_storage(c)
    y[:M] = r["y"].astype(np.float32)
    planes = {n: np.concatenate([r[n], np.full((1, K), B.PLANE_SENTINEL)]) for n in ("x_sign", "x_nz", "x_ste")}
    assert B.y_failures(c, kind, r, y) == [] and B.plane_failures(c, r, planes) == []
    # one weight sign flipped, at the last column some row's input is non-zero in
    o = O - 1
    k = int(np.flatnonzero((r["t"] != 0).any(axis=0) & (d.W[o] != 0))[-1])
    d.W[o, k] = -d.W[o, k]
    bad = B.reference_forward(c, d)
    d.W[o, k] = -d.W[o, k]
    assert np.abs(bad["count"] - r["count"]).max() == 2 and B.y_failures(c, kind, bad, y)
    # a count off by 2 in one element
    bad = dict(r)
    bad["count"] = r["count"].copy()
    bad["count"][M - 1, 0] += 2
    sc, bs = d.scale.astype(np.float64), (0.0 if d.bias is None else d.bias.astype(np.float64))
    bad["y"] = bad["count"] * sc + bs
    bad["mag"] = np.abs(bad["count"] * sc)
    assert len(B.y_failures(c, kind, bad, y)) == 1
    # one plane bit flipped, in each plane
    for n in planes:
        bad = dict(r)
        bad[n] = r[n].copy()
        bad[n][-1, K - 1] ^= np.uint64(1) << np.uint64((M - 1) & 63)
        assert len(B.plane_failures(c, bad, planes)) == 1, n
    # the STE threshold one ulp up, and one ulp down
    for ste in (B.F12_UP, np.nextafter(B.F12, np.float32(0))):
        bad = B.reference_forward(c, d, ste=ste)
        assert [f for f in B.plane_failures(c, bad, planes) if "x_ste" in f], ste
    # guards
    y[M, O - 1] = 0.0
    assert B.y_failures(c, kind, r, y)
    planes["x_nz"][-1, 0] = 0
    assert B.plane_failures(c, r, planes)


def test_column_sum_and_gradient_comparators_have_teeth():
    c = B.by_name(B.I8, "n2_psc7_m63x3")
    for kind in B.KINDS:
        d = B.build_forward(c, kind)
        r = B.reference_forward(c, d)
        ref, mag = R.col_sums(r["count"], d.scale, d.bias)
        y = r["y"]
        assert np.allclose(ref, np.concatenate([y.sum(0), (y * y).sum(0)]), rtol=1e-12, atol=1e-9) and np.all(mag >= np.abs(ref) * (1 - 1e-12))
        assert B.colsum_failures(c, r, d, ref) == []
        bad = ref.copy()
        bad[3] += 2.0 * d.scale[3]                                                # one count off by 2 in one row
        assert B.colsum_failures(c, r, d, bad)
        bad = ref * (1 + 1e-12)
        assert B.colsum_failures(c, r, d, bad)
    for name in ("grad_40x130_a1_e0_s1_b0", "grad_3x63_a0_e0_s0_b0", "grad_5x65_a0_e1_s0_b65"):
        c = B.by_name(B.GRAD, name)
        for kind in B.KINDS:
            d = B.build_grad(c, kind)
            rW, rs, _ = R.weight_grad(d.GX, d.W, d.scale)
            if c["accumulate"]:
                rW, rs = rW + d.dW0, rs + d.dscale0
            dW = None if c["eval"] else rW.astype(np.float32)
            sb = None
            if c["sum_len"]:
                m = c["sum_len"]
                sb = d.sum_store.copy()
                sb[:m] = d.sum_store[m:m + B.RED_SLICES * m].astype(np.float64).reshape(B.RED_SLICES, m).sum(0)
            assert B.grad_failures(c, d, dW, rs.astype(np.float32), sb) == []
            # the 1.2 window one ulp narrower: the planted |W| == 1.2 entries lose their gradient
            if dW is not None and c["O"] * c["K"] >= 64:
                at = np.argwhere((np.abs(d.W) == B.F12) & (rW != 0))
                assert at.size
                bad = dW.copy()
                bad[tuple(at[0])] = 0.0 if not c["accumulate"] else d.dW0[tuple(at[0])]
                assert B.grad_failures(c, d, bad, rs.astype(np.float32), sb)
            bad = rs.astype(np.float32).copy()
            bad[-1] += np.float32(2.0 if kind == "exact" else 0.01 * max(1.0, abs(bad[-1])))
            assert B.grad_failures(c, d, dW, bad, sb)
