"""CPU tests of the ball query's and the grouping's host side: the numpy restatement tests/group_ref.py against the reference's recorded
results (tests/golden/group.npz, written by tests/golden/make_group_golden.py), the contract's order, padding and empty-group rules on
constructed inputs, the argument checks of svnet_amd/group.py, and the pure-host entry points of svnet_amd/csrc/group.hip."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fps_ref as F
from tests import group_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "group.npz"))
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("name", list(G.GOLDEN_CASES))
def test_restatement_equals_the_reference(name):
    seed, B, N, S, nsample, D, radius = G.GOLDEN_CASES[name]
    x, start = GOLDEN[name + "_xyz"], GOLDEN[name + "_start"]
    pts = GOLDEN[name + "_points"] if D else None
    assert x.shape == (B, N, 3) and start.shape == (B,) and ((name + "_points") in GOLDEN.files) == (D > 0)
    bx, bp = G.golden_inputs(name, start)
    assert np.array_equal(_bits(bx), _bits(x)) and (D == 0 or np.array_equal(_bits(bp), _bits(pts)))   # the stored inputs are the procedural ones
    assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    fps = F.fps_batch(x, S, start)
    assert np.array_equal(fps, GOLDEN[name + "_fps"]) and np.array_equal(fps[:, 0], start)
    new_xyz = np.stack([x[b, fps[b]] for b in range(B)])
    assert np.array_equal(_bits(new_xyz), _bits(GOLDEN[name + "_new_xyz"]))
    r2 = G.r2_of(radius)
    idx, count = G.query_ball_batch(x, new_xyz, r2, nsample)
    assert np.array_equal(idx, GOLDEN[name + "_idx"]), name
    assert (count >= 1).all() and count.dtype == np.int32                       # every centre is a point: no empty group
    want = GOLDEN[name + "_new_points"]
    assert want.shape == (B, S, nsample, 3 + D) and want.dtype == F32
    assert np.array_equal(_bits(G.group_batch(x, new_xyz, idx, pts)), _bits(want)), name
    assert np.array_equal(_bits(np.stack([x[b][idx[b]] for b in range(B)])), _bits(GOLDEN[name + "_grouped_xyz"]))
    on_sphere = sum(int((np.take_along_axis(G.distances(new_xyz[b], x[b]), idx[b], axis=1) == r2).any()) for b in range(B))
    if radius in G.EXACT_RADII:
        assert float(r2) == radius * radius and on_sphere == B                  # the planted point of every cloud is in its group
        for b in range(B):
            assert G.planted_index(start[b]) in idx[b, 0]
    else:
        assert on_sphere == 0 and float(r2) * 2 ** 20 != round(float(r2) * 2 ** 20)


def test_golden_holds_every_case_and_both_kinds_of_group():
    want = [n + s for n, c in G.GOLDEN_CASES.items() for s in G.GOLDEN_SUFFIXES if s != "_points" or c[5] > 0]
    assert sorted(GOLDEN.files) == sorted(want)
    assert {c[6] for c in G.GOLDEN_CASES.values()} == {0.125, 0.25, 0.5, 0.1, 0.2, 0.4}
    assert (1, 2048, 128, 32, 3) in {c[1:6] for c in G.GOLDEN_CASES.values()}
    full = partial = 0
    for name, (seed, B, N, S, nsample, D, radius) in G.GOLDEN_CASES.items():
        _, count = G.query_ball_batch(GOLDEN[name + "_xyz"], GOLDEN[name + "_new_xyz"], G.r2_of(radius), nsample)
        full, partial = full + int((count == nsample).sum()), partial + int((count < nsample).sum())
    assert full >= 100 and partial >= 100, (full, partial)                     # the cut and the padding
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "group.npz")) < 512 * 1024


def test_order_cut_padding_and_the_empty_group():
    x = np.zeros((10, 3), dtype=F32)
    x[:, 0] = [0.0, 5.0, 0.5, 1.0, 5.0, -1.0, 0.25, 5.0, 2.0, 1.0]             # distances to the origin: squares of these
    c = np.array([[0, 0, 0], [5, 0, 0], [9, 9, 9], [np.nan, 0, 0]], dtype=F32)
    idx, count = G.query_ball(x, c, F32(1.0), 4)
    assert idx[0].tolist() == [0, 2, 3, 5] and count[0] == 4                   # inside: 0 2 3 5 6 9 (dist == r2 is inside), cut at 4
    assert idx[1].tolist() == [1, 4, 7, 1] and count[1] == 3                   # three found, padded with the first
    assert idx[2].tolist() == [0, 0, 0, 0] and count[2] == 0                   # far from every point: the empty group
    assert idx[3].tolist() == [0, 0, 0, 0] and count[3] == 0                   # a NaN centre: never inside
    idx, count = G.query_ball(x, c[:1], F32(0.99999994), 10)                   # just under 1: the points AT distance 1 drop out
    assert idx[0].tolist() == [0, 2, 6] + [0] * 7 and count[0] == 3
    pts = np.arange(20, dtype=F32).reshape(10, 2)
    out = G.group(x, c[:2], np.array([[0, 2, -5, 13], [1, 4, 7, 1]]), pts)
    assert out.shape == (2, 4, 5)
    assert out[0, :, 0].tolist() == [0.0, 0.5, 0.0, 1.0] and out[1, :, 0].tolist() == [0.0, 0.0, 0.0, 0.0]     # point MINUS centre; clamped
    assert out[0, :, 3:].tolist() == [[0, 1], [4, 5], [0, 1], [18, 19]]
    assert G.group(x, c[:2], np.array([[0], [1]])).shape == (2, 1, 3)


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
def test_procedural_cases(kind):
    make = G.lattice_case if kind == "lattice" else G.gauss_case
    x, c, pts = make(31, 2, 200, 21, 3)
    assert x.shape == (2, 200, 3) and c.shape == (2, 21, 3) and pts.shape == (2, 200, 3) and make(31, 2, 200, 21, 0)[2] is None
    for b in range(2):
        hit = (c[b][:, None, :] == x[b][None, :, :]).all(axis=2).any(axis=1)
        assert hit[0::2].all() and hit.sum() >= 11                             # half of the centres are copies of points
        idx, count = G.query_ball(x[b], c[b], F32(0.0), 4)
        assert (count[hit] >= 1).all() and (count[~hit] == 0).all()            # radius 0: only coincident points are inside
    if kind == "lattice":
        assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    idx, count = G.query_ball(x[0], c[0], G.r2_of(0.4), 8)
    frac = G.scanned_fraction(idx, count, 8, 200)
    assert 0 < frac <= 1


def test_argument_validation_without_a_gpu():
    from svnet_amd import group as Gr
    x, c, pts = (torch.from_numpy(a) for a in G.lattice_case(43, 2, 10, 5, 4))
    idx = torch.zeros(2, 5, 3, dtype=torch.int64)
    for call in (lambda: Gr.query_ball_point(0.2, 3, x, c), lambda: Gr.group_points(x, c, idx, pts), lambda: Gr.group_points(x, c, idx),
                 lambda: Gr.sample_and_group(5, 0.2, 3, x, pts), lambda: Gr.sample_and_group_all(x, pts),
                 lambda: Gr.group_points(x, c, idx, pts, out=torch.empty(2, 5, 3, 7))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        Gr.query_ball_point(0.2, 3, x.numpy(), c)
    with pytest.raises(TypeError):
        Gr.query_ball_point(0.2, 3, x.double(), c)
    with pytest.raises(TypeError):
        Gr.group_points(x, c, idx.int(), pts)
    with pytest.raises(TypeError):
        Gr.group_points(x, c, idx, pts.half())
    with pytest.raises(TypeError):
        Gr.sample_and_group(5, 0.2, 3, x, pts.double())
    with pytest.raises(TypeError):
        Gr.sample_and_group(5, 0.2, 3, x, pts, start=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        Gr.query_ball_point(0.2, 3, x[:, :, :2].contiguous(), c)           # not [B,N,3]
    with pytest.raises(ValueError):
        Gr.query_ball_point(0.2, 3, x, c[:1])                              # batch mismatch
    with pytest.raises(ValueError):
        Gr.query_ball_point(0.2, 3, x[0], c[0])                            # wrong rank
    with pytest.raises(ValueError):
        Gr.query_ball_point(0.2, 3, x.permute(1, 0, 2), c)                 # not contiguous
    with pytest.raises(ValueError):
        Gr.group_points(x, c, idx[:, :4].contiguous(), pts)                # idx's S differs from new_xyz's
    with pytest.raises(ValueError):
        Gr.group_points(x, c, idx, pts[:, :9].contiguous())                # points' N differs from xyz's
    with pytest.raises(ValueError):
        Gr.group_points(x, c, idx, pts.permute(0, 2, 1))                   # wrong shape, not contiguous
    with pytest.raises(ValueError, match="forward only"):
        Gr.group_points(x, c, idx, pts.clone().requires_grad_())
    with pytest.raises(ValueError, match="forward only"):
        Gr.query_ball_point(0.2, 3, x.clone().requires_grad_(), c)
    with pytest.raises(ValueError, match="forward only"):
        Gr.sample_and_group(5, 0.2, 3, x.clone().requires_grad_(), pts)
    with pytest.raises(ValueError):
        Gr.group_points(x, c, idx, pts.to("meta"))                         # mismatched devices
    with pytest.raises(RuntimeError):
        Gr.Grouper(2, 10, 5, 3, 4, "cpu")


def test_header_binding_and_library_agree():
    from svnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "svnet_hip.h")).read()
    new = ("svnet_group_supported", "svnet_ball_query_tile", "svnet_ball_query_f32", "svnet_group_points_f32")
    for name in new:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert len(_lib.SIGNATURES["svnet_ball_query_f32"][1]) == 10 and len(_lib.SIGNATURES["svnet_group_points_f32"][1]) == 11
    assert _lib.SIGNATURES["svnet_ball_query_f32"][1][5] is _lib.c_f       # r2 is an fp32 argument
    header_abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert L.svnet_version() == _lib.ABI_VERSION == header_abi and header_abi >= 422         # bumped with the new entry points
    assert "422: svnet_ball_query_f32" in header                                            # and listed in the header's change list


def test_supported_query_and_refusals_without_a_gpu():
    import ctypes
    from svnet_amd import _lib, group as Gr
    L = _lib.lib()
    for N, S, ns, D in ((1, 1, 1, 0), (32768, 1, 1, 0), (2048, 512, 64, 67)):
        assert L.svnet_group_supported(N, S, ns, D) == 1, (N, S, ns, D)
    for N, S, ns, D in ((5, 1, 6, 0), (0, 1, 1, 0), (32769, 1, 1, 0), (5, 0, 1, 0), (5, 1, 1, -1), (5, 1, 0, 0), (-3, 1, 1, 0)):
        assert L.svnet_group_supported(N, S, ns, D) == 0, (N, S, ns, D)
    tile = Gr.tile()
    assert tile >= 64 and tile % 64 == 0 and tile * 12 <= 64 * 1024             # an LDS tile without an opt-in, whole 64-candidate steps
    p = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused on the host
    q, g = L.svnet_ball_query_f32, L.svnet_group_points_f32
    assert q(None, p, 1, 8, 4, 0.04, 2, p, p, None) == -1 and b"null" in L.svnet_last_error()
    assert q(p, p, 1, 8, 4, 0.04, 2, p, None, None) == -1
    assert q(p, p, 0, 8, 4, 0.04, 2, p, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert q(p, p, 1, 8, 4, 0.04, 9, p, p, None) == -2 and b"nsample" in L.svnet_last_error()
    assert q(p, p, 1, 32769, 4, 0.04, 2, p, p, None) == -2 and b"32768" in L.svnet_last_error()
    assert q(p, p, 1, 8, 0, 0.04, 2, p, p, None) == -2
    assert q(p, p, 1 << 31, 8, 4, 0.04, 2, p, p, None) == -2 and b"2^31" in L.svnet_last_error()
    assert g(p, None, p, p, 1, 8, 4, 2, 3, p, None) == -1 and b"null" in L.svnet_last_error()
    assert g(p, p, None, p, 1, 8, 4, 2, 3, p, None) == -1 and b"null points" in L.svnet_last_error()       # D > 0 needs points
    assert g(p, p, p, p, 0, 8, 4, 2, 3, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert g(p, p, p, p, 1, 8, 4, 9, 3, p, None) == -2 and b"nsample" in L.svnet_last_error()
    assert g(p, p, p, p, 1, 8, 4, 2, -1, p, None) == -2
    assert g(p, p, p, p, 1 << 29, 8, 4, 2, 3, p, None) == -2 and b"2^31" in L.svnet_last_error()
