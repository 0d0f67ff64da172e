"""CPU tests of the feature propagation's host side: the numpy restatement tests/propagate_ref.py against the reference's recorded
results (tests/golden/propagate.npz, written by tests/golden/make_propagate_golden.py), the contract's tie rule and small-N semantics
on constructed inputs, the argument checks of svnet_amd/propagate.py, and the pure-host entry points of svnet_amd/csrc/propagate.hip."""
import os
import re

import numpy as np
import pytest
import torch

from tests import propagate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "propagate.npz"))
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_equals_the_reference(name):
    seed, B, P, N, D = R.GOLDEN_CASES[name]
    q, r, f = GOLDEN[name + "_q"], GOLDEN[name + "_r"], GOLDEN[name + "_f"]
    assert q.shape == (B, P, 3) and r.shape == (B, N, 3) and f.shape == (B, D, N)
    built = R.lattice_case(seed, B, P, N, D)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(built, (q, r, f)))        # the stored inputs are the procedural ones
    assert np.array_equal(q * 1024, np.round(q * 1024)) and abs(q).max() <= 1 and abs(r).max() <= 1
    assert R.distinct_smallest(q, r)
    idx, dist3, _ = R.three_nn_batch(q, r)
    if N >= 3:
        assert np.array_equal(idx, GOLDEN[name + "_idx"]), name
    else:
        assert name + "_idx" not in GOLDEN.files
    assert (dist3[:, :, 0] == 0).any()                                                       # coincident points are in
    want = GOLDEN[name + "_out"]
    assert want.shape == (B, D, P) and want.dtype == F32
    assert np.array_equal(_bits(R.propagate_batch(q, r, f)), _bits(want)), name


def test_golden_holds_every_case():
    want = [n + s for n, c in R.GOLDEN_CASES.items() for s in ("_q", "_r", "_f", "_out") + (("_idx",) if c[3] >= 3 else ())]
    assert sorted(GOLDEN.files) == sorted(want)
    shapes = {c[1:] for c in R.GOLDEN_CASES.values()}
    assert {(2, 200, 37, 5), (2, 300, 3, 4), (1, 64, 2049, 3)} <= shapes and any(s[2] == 1 for s in shapes)


def test_tie_rule_lower_index_first():
    q = np.zeros((2, 3), dtype=F32)
    same = np.tile(np.array([[0.5, -0.25, 1.0]], dtype=F32), (6, 1))
    idx, dist3, w = R.three_nn(q, same)                                   # all sampled points identical: 0, 1, 2
    assert (idx == [0, 1, 2]).all() and (dist3 == dist3[0, 0]).all()
    assert (w == w[0, 0]).all() and abs(float(w[0, 0]) - 1 / 3) < 1e-6
    # ring of equidistant points around the query with one nearer point at the end: nearer first, then the two lowest indices
    r = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, 0.5, 0]], dtype=F32)
    idx, dist3, _ = R.three_nn(q[:1], r)
    assert idx.tolist() == [[4, 0, 1]] and dist3.tolist() == [[0.25, 1.0, 1.0]]
    # a duplicated pair: the lower index of the pair first, wherever the pair lies
    r = np.array([[3, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0, 0]], dtype=F32)
    assert R.three_nn(q[:1], r)[0].tolist() == [[1, 3, 2]]


@pytest.mark.parametrize("N", [1, 2, 3])
def test_small_n_semantics(N):
    q = np.array([[0.1, 0.2, 0.3], [1.0, -1.0, 0.5], [0.0, 0.0, 0.0]], dtype=F32)
    r = np.array([[0.0, 0.0, 0.0], [1.0, -1.0, 0.25], [0.3, 0.2, 0.1]], dtype=F32)[:N]
    f = np.array([[1.5, -2.0, 4.0], [0.25, 8.0, -1.0]], dtype=F32)[:, :N]
    idx, dist3, w = R.three_nn(q, r)
    assert ((idx >= 0) & (idx < N)).all()
    assert (idx[:, N:] == 0).all() and np.isinf(dist3[:, N:]).all() and (w[:, N:] == 0).all()       # slots past K
    assert np.isfinite(dist3[:, :N]).all() and (np.diff(dist3[:, :N], axis=1) >= 0).all()
    assert sorted(idx[0, :N].tolist()) == list(range(N))
    out = R.three_interpolate(f, idx, w)
    if N == 1:
        assert (w[:, 0] == 1).all() and np.array_equal(_bits(out), _bits(np.repeat(f, 3, axis=1)))  # the reference's S == 1 branch
    assert idx[2, 0] == 0 and dist3[2, 0] == 0 and abs(out[0, 2] - f[0, 0]) < 1e-5     # the query AT sampled point 0 takes its value
    lo, hi = f.min(axis=1, keepdims=True), f.max(axis=1, keepdims=True)
    assert (out >= lo - 1e-4).all() and (out <= hi + 1e-4).all()               # a convex combination


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
def test_weights_distances_and_the_float64_form(kind):
    make = R.lattice_case if kind == "lattice" else R.gauss_case
    q, r, f = make(41, 2, 300, 129, 6)
    for b in range(2):
        idx, dist3, w = R.three_nn(q[b], r[b])
        assert (dist3 >= 0).all() and not np.signbit(dist3).any()             # never negative, not even -0
        hit = (q[b][:, None, :] == r[b][None, :, :]).all(axis=2).any(axis=1)  # queries that coincide with a sampled point
        assert hit.sum() >= 64 and (dist3[hit, 0] == 0).all() and (dist3[~hit, 0] > 0).all()
        s = w.astype(np.float64).sum(axis=1)
        assert (abs(s - 1.0) <= 2 * 2.0 ** -23).all(), abs(s - 1.0).max()     # within 2 ulp of 1
        assert (w >= 0).all() and (np.diff(w, axis=1) <= 0).all()             # nearer neighbours weigh more
        out = R.three_interpolate(f[b], idx, w)
        err, bound = float(abs(out - R.interpolate_f64(q[b], r[b], f[b], idx)).max()), R.bound_f32(f[b])
        print("%s cloud %d: |fp32 - f64| %.3e, bound %.3e (%.2f of it)" % (kind, b, err, bound, err / bound))
        assert err <= bound, (err, bound)


def test_expanded_form_is_not_the_contract():
    """Why the contract does not copy the reference's -2 q.r + |q|^2 + |r|^2: at a coincident Gaussian point it is not 0."""
    q, r, _ = R.gauss_case(42, 1, 200, 64, 1)
    tq, tr = torch.from_numpy(q), torch.from_numpy(r)
    expanded = -2 * torch.matmul(tq, tr.permute(0, 2, 1)) + (tq ** 2).sum(-1)[:, :, None] + (tr ** 2).sum(-1)[:, None, :]
    same = np.arange(32)
    assert (expanded[0, same, same] != 0).any()
    assert (R.distances(q[0], r[0])[same, same] == 0).all()


def test_argument_validation_without_a_gpu():
    from svnet_amd import propagate as Pr
    q, r, f = (torch.from_numpy(a) for a in R.lattice_case(43, 2, 10, 5, 4))
    idx, w = torch.zeros(2, 10, 3, dtype=torch.int64), torch.zeros(2, 10, 3)
    for call in (lambda: Pr.three_nn(q, r), lambda: Pr.three_interpolate(f, idx, w), lambda: Pr.propagate(q, r, f),
                 lambda: Pr.propagate(q, r, f, out=torch.empty(2, 4, 10))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        Pr.three_nn(q.numpy(), r)
    with pytest.raises(TypeError):
        Pr.three_nn(q.double(), r)
    with pytest.raises(TypeError):
        Pr.three_interpolate(f, idx.int(), w)
    with pytest.raises(TypeError):
        Pr.three_interpolate(f, idx, w.double())
    with pytest.raises(TypeError):
        Pr.propagate(q, r, f.half())
    with pytest.raises(TypeError):
        Pr.propagate(q, r, None)
    with pytest.raises(ValueError):
        Pr.three_nn(q[:, :, :2].contiguous(), r)                       # not [B,P,3]
    with pytest.raises(ValueError):
        Pr.three_nn(q, r[:1])                                          # batch mismatch
    with pytest.raises(ValueError):
        Pr.three_nn(q.permute(1, 0, 2), r)                             # not contiguous
    with pytest.raises(ValueError):
        Pr.three_interpolate(f, idx[:, :, :2].contiguous(), w)
    with pytest.raises(ValueError):
        Pr.three_interpolate(f, idx, w[:, :5].contiguous())
    with pytest.raises(ValueError):
        Pr.propagate(q, r, f[:, :, :4].contiguous())                   # feat's N differs from ref's
    with pytest.raises(ValueError):
        Pr.propagate(q, r, f.clone().requires_grad_())                 # forward only
    with pytest.raises(ValueError):
        Pr.propagate(q, r, f.to("meta"))                               # mismatched devices
    with pytest.raises(RuntimeError):
        Pr.Propagator(2, 4, 5, 10, "cpu")


def test_header_binding_and_library_agree():
    from svnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "svnet_hip.h")).read()
    new = ("svnet_propagate_supported", "svnet_three_nn_f32", "svnet_three_interpolate_f32")
    for name in new:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert len(_lib.SIGNATURES["svnet_three_nn_f32"][1]) == 9 and len(_lib.SIGNATURES["svnet_three_interpolate_f32"][1]) == 9
    header_abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert L.svnet_version() == _lib.ABI_VERSION == header_abi and header_abi > 420        # bumped with the new entry points


def test_supported_query_and_refusals_without_a_gpu():
    import ctypes
    from svnet_amd import _lib, propagate as Pr
    L = _lib.lib()
    for P, N, D in ((1, 1, 1), (10000, 2048, 50), (1 << 33, 32768, 1 << 20)):
        assert L.svnet_propagate_supported(P, N, D) == 1, (P, N, D)
    for P, N, D in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 32769, 1), (-1, 5, 5), (1 << 40, 5, 5)):
        assert L.svnet_propagate_supported(P, N, D) == 0, (P, N, D)
    tile = Pr.tile()
    assert tile >= 64 and tile % 4 == 0 and tile * 12 <= 64 * 1024             # an LDS tile without an opt-in
    p = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused on the host
    assert L.svnet_three_nn_f32(None, p, 1, 8, 4, p, p, p, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_three_nn_f32(p, p, 1, 8, 4, p, None, p, None) == -1
    assert L.svnet_three_nn_f32(p, p, 0, 8, 4, p, p, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert L.svnet_three_nn_f32(p, p, 1, 8, 32769, p, p, p, None) == -2 and b"32768" in L.svnet_last_error()
    assert L.svnet_three_nn_f32(p, p, 1 << 31, 8, 4, p, p, p, None) == -2 and b"2^31" in L.svnet_last_error()
    assert L.svnet_three_interpolate_f32(p, p, None, 1, 2, 4, 8, p, None) == -1 and b"null" in L.svnet_last_error()
    assert L.svnet_three_interpolate_f32(p, p, p, 1, 0, 4, 8, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert L.svnet_three_interpolate_f32(p, p, p, 1, 2, 32769, 8, p, None) == -2 and b"32768" in L.svnet_last_error()
    assert L.svnet_three_interpolate_f32(p, p, p, 1 << 31, 2, 4, 8, p, None) == -2


def test_source_points_refuses_what_is_not_a_pool():
    from svnet_amd import propagate as Pr
    with pytest.raises(TypeError):
        Pr.source_points(object(), object())
