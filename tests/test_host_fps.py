"""CPU tests of farthest point sampling's host side: the numpy restatement tests/fps_ref.py against the reference's recorded results
(tests/golden/fps.npz, written by tests/golden/make_fps_golden.py), the counter-based start, and the pure-host entry points of
svnet_amd/csrc/fps.hip."""
import os

import numpy as np
import pytest

from tests import fps_ref as F

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fps.npz"))


@pytest.mark.parametrize("name", list(F.golden_cases()))
def test_restatement_equals_the_reference(name):
    clouds, npoint = F.golden_cases()[name]
    want = GOLDEN["fps_" + name]
    assert want.shape == (clouds.shape[0], npoint) and want.dtype == np.int64
    assert np.isfinite(clouds).all()
    got = F.fps_batch(clouds, npoint, want[:, 0])
    assert np.array_equal(got, want), name


def test_golden_holds_every_case_and_the_modelnet_shape():
    assert sorted(GOLDEN.files) == sorted(["fps_" + n for n in F.golden_cases()] + ["norm_" + n for n in F.norm_cases()])
    assert GOLDEN["fps_modelnet_v2"].shape == (2, 1024) and F.golden_cases()["modelnet_v2"][0].shape == (2, 10000, 3)
    rep = GOLDEN["fps_repeated40"][0]
    assert (rep[8:] == 0).all() and len(set(rep[:8].tolist())) == 8          # 8 distinct points, then index 0 for ever
    full = GOLDEN["fps_full65"]
    assert all(sorted(row.tolist()) == list(range(65)) for row in full)      # npoint == P of distinct points: a permutation


def test_fps_start_is_a_pure_function_in_range():
    from svnet_amd.data import fps_start
    from svnet_amd import synth
    a = fps_start(3, 100, 10000)
    assert a.dtype == np.int64 and a.shape == (100,) and (a >= 0).all() and (a < 10000).all()
    assert np.array_equal(a, fps_start(3, 100, 10000))
    assert np.array_equal(a[:10], fps_start(3, 10, 10000))                    # cloud m's start does not depend on M
    assert not np.array_equal(a, fps_start(4, 100, 10000)) and len(set(a.tolist())) > 90
    sm = lambda v: synth._splitmix64(np.asarray(v, dtype=np.uint64))          # noqa: E731
    assert int(a[7]) == int(sm(sm(np.uint64(3)) ^ np.uint64(7)) % np.uint64(10000))
    assert (fps_start(0, 50, 1) == 0).all()
    with pytest.raises(ValueError):
        fps_start(0, 0, 5)


def test_supported_and_tier_queries():
    from svnet_amd import _lib
    L = _lib.lib()
    for P, n in ((1, 1), (10000, 1024), (16384, 16384)):
        assert L.svnet_fps_supported(P, n) == 1, (P, n)
    for P, n in ((0, 1), (5, 0), (5, 6), (16385, 1), (-1, 1)):
        assert L.svnet_fps_supported(P, n) == 0, (P, n)
    tiers = [L.svnet_fps_tier(P) for P in range(0, 16386)]
    assert tiers[0] == -1 and tiers[16385] == -1 and L.svnet_fps_tier(-7) == -1 and L.svnet_fps_tier(1 << 40) == -1
    inside = tiers[1:16385]
    assert inside[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(inside, inside[1:]))      # 0 .. n-1, non-decreasing in P, none skipped
    for P in (1, 2, 64, 65, 4097, 16384):
        assert (L.svnet_fps_tier(P) >= 0) == bool(L.svnet_fps_supported(P, 1))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from svnet_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused on the host
    assert L.svnet_fps_f32(None, 1, 8, 4, p, p, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_fps_f32(p, 1, 8, 4, None, p, None) == -1
    assert L.svnet_fps_f32(p, 1, 8, 4, p, None, None) == -1
    assert L.svnet_fps_f32(p, 0, 8, 4, p, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert L.svnet_fps_f32(p, 1, 8, 9, p, p, None) == -1 and b"npoint 9 > P 8" in L.svnet_last_error()
    assert L.svnet_fps_f32(p, 1, 16385, 4, p, p, None) < 0 and b"16384" in L.svnet_last_error()
    assert L.svnet_pool_gather_f32(None, None, p, 1, 8, 4, 0, p, None, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_pool_gather_f32(p, None, p, 1, 8, 4, 0, p, p, None) == -1 and b"seg" in L.svnet_last_error()
    assert L.svnet_pool_gather_f32(p, None, p, 1, 0, 4, 0, p, None, None) == -1


@pytest.mark.parametrize("name", list(F.norm_cases()))
def test_float64_normalise_is_the_reference_function(name):
    """|float64 restatement - the reference's recorded float32 pc_normalize| <= 2^-24 (8 + 2 N ||p||inf / m): the worst case of
    numpy's sequential fp32 mean entering d and m.  Loose on purpose: a wrong axis or a missing sqrt misses it by orders of magnitude."""
    sel = F.norm_cases()[name]
    want = GOLDEN["norm_" + name]
    assert want.dtype == np.float32 and want.shape == sel.shape and sel.shape[0] <= 128
    err, bound = float(abs(F.normalize_f64(sel) - want).max()), F.bound_numpy_f32(sel)
    print("%s: |f64 - reference| %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name", list(F.norm_cases()))
def test_fp32_normalise_is_within_its_derived_bound(name):
    """The fp32 sequence the kernel runs (restated) against float64: 2^-24 (8 + 4 ||c||inf / m)."""
    sel = F.norm_cases()[name]
    got = F.normalize_f32(sel)
    err, bound = float(abs(F.normalize_f64(sel) - got).max()), F.bound_f32(sel)
    print("%s: |f64 - fp32| %.3e, bound %.3e (%.2f of it)" % (name, err, bound, err / bound))
    assert got.dtype == np.float32 and err <= bound, (name, err, bound)
    assert abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)).max() - 1.0) < 1e-6
    # the fixed-order float64 mean against numpy's own float64 mean: the same value up to the final rounding to fp32
    assert np.allclose(F.centroid_f32(sel), sel.astype(np.float64).mean(axis=0), rtol=2.0 ** -23, atol=0.0)
