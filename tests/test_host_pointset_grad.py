"""CPU tests of the host side of the grouping and interpolation gradients: the numpy restatement tests/pointset_grad_ref.py against
the reference's recorded gradients (tests/golden/pointset_grad.npz, written by tests/golden/make_pointset_grad_golden.py), the
pure-host entry points of svnet_amd/csrc/pointset_grad.hip, the argument checks, and the state_dict layout of the modules of
svnet_amd/models/utils/pointnet_util.py."""
import os
import re

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import group_ref as G
from tests import pointset_grad_ref as PG
from tests import propagate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "pointset_grad.npz"))
GROUP_GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "group.npz"))
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_reverse_lists_on_a_constructed_table():
    idx = np.array([[2, 0, 2], [7, -3, 2], [1, 1, 0]], dtype=np.int64)         # 7 and -3 are clamped into [0, 4)
    start, edge = PG.reverse_lists(idx, 4)
    assert start.tolist() == [0, 3, 5, 8, 9] and edge.tolist() == [1, 4, 8, 6, 7, 0, 2, 5, 3]
    assert start.dtype == np.int32 and edge.dtype == np.int32
    start, edge = PG.reverse_lists(idx, 1)                                      # one point takes every edge, in order
    assert start.tolist() == [0, 9] and edge.tolist() == list(range(9))
    start, edge = PG.reverse_lists(idx[:1], 6)                                  # empty lists
    assert start.tolist() == [0, 1, 1, 3, 3, 3, 3] and edge.tolist() == [1, 0, 2]


def test_ordered_sum_is_the_contracts_association():
    big, one = F32(2.0 ** 24), F32(1.0)
    terms = np.array([[one, big, -big, one, -0.0]], dtype=F32)
    idx = np.array([[0, 0, 0, 0, 2]], dtype=np.int64)
    out = PG.ordered_sums(terms, *PG.reverse_lists(idx, 4))
    assert out[0, 0] == 1.0                                                     # ((1 + 2^24) - 2^24) + 1: the first 1 is lost
    assert _bits(out[0, 2]) == 0x80000000                                       # one term gives the term itself: -0 stays
    assert _bits(out[0, 1]) == 0 and _bits(out[0, 3]) == 0                      # no term: +0
    exact, bound = PG._sums_f64(terms.astype(np.float64), idx, 4)
    assert exact[0, 0] == 2.0 and abs(float(out[0, 0]) - exact[0, 0]) <= bound[0, 0]


@pytest.mark.parametrize("name", PG.GROUP_CASES)
def test_grouping_restatement_equals_the_reference(name):
    seed, B, N, S, nsample, D, _ = G.GOLDEN_CASES[name]
    g, want, idx = GOLDEN["ga_%s_g" % name], GOLDEN["ga_%s_dpoints" % name], GROUP_GOLDEN[name + "_idx"]
    assert g.shape == (B, S, nsample, 3 + D) and g.dtype == np.int8 and abs(g).max() <= 4 and want.shape == (B, N, D) and want.dtype == F32
    assert np.array_equal(g, (synth.integers(seed, 7, g.shape, 9) - 4).astype(np.int8))          # the stored gradient is the procedural one
    assert np.array_equal(_bits(PG.group_bwd_batch(g.astype(F32), idx, N)), _bits(want)), name
    exact, bound = PG.group_bwd_f64(g[0], idx[0], N)
    assert np.array_equal(exact, want[0]) and (bound >= 0).all()                                 # integer sums: exact in both


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_interpolation_restatement_within_the_bound_of_the_reference(name):
    seed, B, P, N, D = R.GOLDEN_CASES[name]
    q, r, _ = R.lattice_case(seed, B, P, N, D)
    dout, want = GOLDEN["gb_%s_dout" % name], GOLDEN["gb_%s_dfeat" % name]
    assert dout.shape == (B, D, P) and want.shape == (B, D, N) and want.dtype == F32
    assert np.array_equal(_bits(dout), _bits(synth.normal(seed, 5, (B, D, P))))
    idx, _, w = R.three_nn_batch(q, r)
    mine = PG.interpolate_bwd_batch(dout, idx, w, N)
    for b in range(B):
        exact, bound = PG.interpolate_bwd_f64(dout[b], idx[b], w[b], N)
        for a in (mine[b], want[b]):
            assert (np.abs(a - exact) <= bound).all(), name
    # the adjoint identity of the restatements: <interpolate(f), g> = <f, interpolate_bwd(g)>
    f = synth.normal(seed, 4, (B, D, N)).astype(np.float64)
    lhs = sum(float((R.three_interpolate(f[b], idx[b], w[b]).astype(np.float64) * dout[b]).sum()) for b in range(B))
    rhs = float((f * mine).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), 1.0), (lhs, rhs)


def test_golden_holds_every_entry():
    files = set(GOLDEN.files)
    want = {"ga_%s_%s" % (n, s) for n in PG.GROUP_CASES for s in ("g", "dpoints")}
    want |= {"gb_%s_%s" % (n, s) for n in R.GOLDEN_CASES for s in ("dout", "dfeat")}
    assert want <= files and all(G.GOLDEN_CASES[n][5] > 0 for n in PG.GROUP_CASES)
    for key in ("gc_xyz", "gc_feat", "gc_lw", "gc_start", "gc_keys", "gc_shapes", "gc_out:loss", "gc_out:u0", "gc_dx:feat"):
        assert key in files, key
    keys = [str(k) for k in GOLDEN["gc_keys"]]
    assert {"gc_sd:" + k for k in keys} <= files
    assert {"gc_d:" + k for k in keys if k.endswith(("weight", "bias"))} <= files               # every parameter's gradient
    c = PG.STACK
    assert GOLDEN["gc_xyz"].shape == (c["B"], 3, c["N"]) and GOLDEN["gc_feat"].shape == (c["B"], c["D"], c["N"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointset_grad.npz")) < 300 * 1024


def test_supported_and_tile_queries_without_a_gpu():
    import ctypes
    from svnet_amd import _lib, _pointset
    L = _lib.lib()
    for R_, K, N in ((1, 1, 1), (10000, 3, 2048), (512, 64, 32768), ((1 << 31) - 1, 1, 5), (1 << 29, 3, 5)):
        assert L.svnet_pointset_reverse_supported(R_, K, N) == 1, (R_, K, N)
    for R_, K, N in ((0, 3, 5), (5, 0, 5), (5, 3, 0), (5, 3, 32769), (1 << 31, 1, 5), (1 << 30, 3, 5), (-1, 3, 5)):
        assert L.svnet_pointset_reverse_supported(R_, K, N) == 0, (R_, K, N)
    tile = _pointset.reverse_tile()
    assert tile >= 64 and tile % 64 == 0 and tile <= 1024                       # whole waves of one workgroup
    chunk = _pointset.reverse_chunk()
    assert chunk >= tile and chunk % tile == 0 and chunk * 4 <= 64 * 1024       # an LDS chunk without an opt-in, staged in whole steps
    p = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused on the host
    rev, ib, gb = L.svnet_pointset_reverse_i32, L.svnet_three_interpolate_bwd_f32, L.svnet_group_points_bwd_f32
    assert rev(None, 1, 4, 3, 5, p, p, None) == -1 and b"null" in L.svnet_last_error()
    assert rev(p, 0, 4, 3, 5, p, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert rev(p, 1, 4, 3, 32769, p, p, None) == -2 and b"32768" in L.svnet_last_error()
    assert rev(p, 1, 1 << 31, 3, 5, p, p, None) == -2 and b"2^31" in L.svnet_last_error()
    assert ib(p, None, p, p, 1, 2, 5, 4, p, None) == -1 and b"null" in L.svnet_last_error()
    assert ib(p, p, p, p, 0, 2, 5, 4, p, None) == -1
    assert ib(p, p, p, p, 1, 0, 5, 4, p, None) == -2 and ib(p, p, p, p, 1, 2, 32769, 4, p, None) == -2
    assert gb(p, p, None, 1, 5, 4, 3, 2, p, None) == -1 and b"null" in L.svnet_last_error()
    assert gb(p, p, p, 1, 5, 4, 3, 0, p, None) == -2 and gb(p, p, p, 1, 0, 4, 3, 2, p, None) == -2
    header = open(os.path.join(ROOT, "include", "svnet_hip.h")).read()
    for name in ("svnet_pointset_reverse_supported", "svnet_pointset_reverse_tile", "svnet_pointset_reverse_chunk", "svnet_pointset_reverse_i32",
                 "svnet_three_interpolate_bwd_f32", "svnet_group_points_bwd_f32"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION >= 425 and "425: svnet_pointset_reverse_i32" in header


def test_argument_errors_without_a_gpu():
    from svnet_amd import group as Gr, propagate as Pr
    q, r, f = (torch.from_numpy(a) for a in R.lattice_case(43, 2, 10, 5, 4))
    x, c, pts = (torch.from_numpy(a) for a in G.lattice_case(43, 2, 10, 5, 4))
    idx3, w3 = torch.zeros(2, 10, 3, dtype=torch.int64), torch.zeros(2, 10, 3)
    gidx = torch.zeros(2, 5, 3, dtype=torch.int64)
    # a grad on coordinates, weights and indices' companions is refused whatever the device
    for call in (lambda: Pr.propagate(q.clone().requires_grad_(), r, f), lambda: Pr.propagate(q, r.clone().requires_grad_(), f),
                 lambda: Pr.three_interpolate(f, idx3, w3.clone().requires_grad_()),
                 lambda: Gr.group_points(x.clone().requires_grad_(), c, gidx, pts), lambda: Gr.group_points(x, c.clone().requires_grad_(), gidx, pts),
                 lambda: Gr.sample_and_group(5, 0.2, 3, x.clone().requires_grad_(), pts), lambda: Gr.sample_and_group_all(x.clone().requires_grad_(), pts),
                 lambda: Gr.Grouper.run(None, x, c, 0.2, pts.clone().requires_grad_()),
                 lambda: Pr.three_interpolate_backward(f.clone().requires_grad_(), idx3, w3, 5),
                 lambda: Gr.group_points_backward(torch.zeros(2, 5, 3, 7).requires_grad_(), gidx, 10)):
        with pytest.raises(ValueError, match="requires grad"):
            call()
    # the data tensors may require grad only where the backward exists: on a HIP device
    for call in (lambda: Pr.propagate(q, r, f.clone().requires_grad_()), lambda: Pr.three_interpolate(f.clone().requires_grad_(), idx3, w3),
                 lambda: Gr.group_points(x, c, gidx, pts.clone().requires_grad_()), lambda: Gr.sample_and_group(5, 0.2, 3, x, pts.clone().requires_grad_()),
                 lambda: Gr.sample_and_group_all(x, pts.clone().requires_grad_())):
        with pytest.raises(ValueError, match="off a HIP device"):
            call()
    # the functional backwards: no CPU fallback, and their shape checks
    for call in (lambda: Pr.three_interpolate_backward(torch.zeros(2, 4, 10), idx3, w3, 5), lambda: Gr.group_points_backward(torch.zeros(2, 5, 3, 7), gidx, 10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        Pr.three_interpolate_backward(torch.zeros(2, 4, 11), idx3, w3, 5)          # dout's P differs from idx's
    with pytest.raises(ValueError):
        Gr.group_points_backward(torch.zeros(2, 5, 3, 3), gidx, 10)                # D = 0: there is nothing to differentiate
    with pytest.raises(ValueError):
        Gr.group_points_backward(torch.zeros(2, 5, 4, 7), gidx, 10)
    with pytest.raises(TypeError):
        Gr.group_points_backward(torch.zeros(2, 5, 3, 7), gidx.int(), 10)


def test_out_beside_a_grad_is_refused(monkeypatch):
    """`out=` together with an input that requires grad raises a ValueError before anything is launched.  Without a GPU the two
    device checks in front of that refusal are patched to let CPU tensors through (tests/test_hip_pointset_grad.py sees the same
    refusal unpatched)."""
    from svnet_amd import _call, _pointset, group as Gr, propagate as Pr
    real = _pointset.check_tensors

    def lenient(name, tensors, dtypes, what, grad=()):
        real(name, {k: (t.detach() if isinstance(t, torch.Tensor) and k in grad else t) for k, t in tensors.items()}, dtypes, what, grad)
        return any(tensors[k].requires_grad for k in grad if k in tensors)

    monkeypatch.setattr(_pointset, "check_tensors", lenient)
    monkeypatch.setattr(_call, "hip", lambda *t: None)
    q, r, f = (torch.from_numpy(a) for a in R.lattice_case(43, 2, 10, 5, 4))
    x, c, pts = (torch.from_numpy(a) for a in G.lattice_case(43, 2, 10, 5, 4))
    idx3, w3, gidx = torch.zeros(2, 10, 3, dtype=torch.int64), torch.zeros(2, 10, 3), torch.zeros(2, 5, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="out="):
        Pr.propagate(q, r, f.clone().requires_grad_(), out=torch.empty(2, 4, 10))
    with pytest.raises(ValueError, match="out="):
        Pr.three_interpolate(f.clone().requires_grad_(), idx3, w3, out=torch.empty(2, 4, 10))
    with pytest.raises(ValueError, match="out="):
        Gr.group_points(x, c, gidx, pts.clone().requires_grad_(), out=torch.empty(2, 5, 3, 7))


def _modules():
    from svnet_amd.models.utils import pointnet_util as U
    return U, PG.stack_modules(U)


def test_module_state_dicts_equal_the_recorded_layout():
    U, mods = _modules()
    keys = [str(k) for k in GOLDEN["gc_keys"]]
    shapes = [tuple(int(v) for v in row if v >= 0) for row in GOLDEN["gc_shapes"]]
    mine = [("%s.%s" % (m, k), tuple(v.shape)) for m, mod in mods.items() for k, v in mod.state_dict().items()]
    assert mine == list(zip(keys, shapes))
    assert isinstance(mods["sa1"].mlp_convs[0], torch.nn.Conv2d) and isinstance(mods["fp1"].mlp_convs[0], torch.nn.Conv1d)
    assert isinstance(mods["sa1"].mlp_bns[0], torch.nn.BatchNorm2d) and isinstance(mods["fp1"].mlp_bns[0], torch.nn.BatchNorm1d)
    for name in ("farthest_point_sample", "query_ball_point", "sample_and_group", "sample_and_group_all"):
        assert callable(getattr(U, name)), name
    assert not hasattr(U, "PointNetSetAbstractionMsg")


def test_recorded_state_dict_loads_strictly():
    _, mods = _modules()
    for m, mod in mods.items():
        state = {k[len("gc_sd:") + len(m) + 1:]: torch.from_numpy(GOLDEN[k]) for k in GOLDEN.files if k.startswith("gc_sd:%s." % m)}
        assert state
        mod.load_state_dict(state, strict=True)
        for k, v in mod.state_dict().items():
            assert torch.equal(v, state[k]), (m, k)


def test_module_signatures_are_the_references():
    import inspect
    U, _ = _modules()
    assert list(inspect.signature(U.PointNetSetAbstraction.__init__).parameters)[1:] == ["npoint", "radius", "nsample", "in_channel", "mlp", "group_all"]
    assert list(inspect.signature(U.PointNetFeaturePropagation.__init__).parameters)[1:] == ["in_channel", "mlp"]
    assert list(inspect.signature(U.PointNetSetAbstraction.forward).parameters)[1:] == ["xyz", "points", "start"]
    assert list(inspect.signature(U.PointNetFeaturePropagation.forward).parameters)[1:] == ["xyz1", "xyz2", "points1", "points2"]
