"""CPU tests of the multi-scale grouping's host side: the numpy restatement tests/msg_ref.py against the reference's recorded results
(tests/golden/msg.npz, written by tests/golden/make_msg_golden.py), the layout and sum order of the contract on constructed inputs,
the new names in the parsed header, the pure-host refusals of svnet_amd/csrc/group.hip, and the argument checks of
svnet_amd/group.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import fps_ref as F
from tests import group_ref as G
from tests import msg_ref as M
from tests import pointset_grad_ref as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "msg.npz"))
F32 = np.float32
NEW = ("svnet_group_msg_supported", "svnet_ball_query_msg_f32", "svnet_group_points_msg_f32", "svnet_group_points_msg_bwd_f32")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("name", list(M.GOLDEN_CASES))
def test_restatement_equals_the_reference(name):
    seed, B, N, S, radii, nsamples, D, mlp_list = M.GOLDEN_CASES[name]
    R = len(radii)
    x, start = GOLDEN[name + "_xyz"], GOLDEN[name + "_start"]
    pts = GOLDEN[name + "_points"] if D else None
    assert x.shape == (B, N, 3) and N <= 256 and S <= 32 and B == 2 and ((name + "_points") in GOLDEN.files) == (D > 0)
    bx, bp = M.golden_inputs(name, start)
    assert np.array_equal(_bits(bx), _bits(x)) and (D == 0 or np.array_equal(_bits(bp), _bits(pts)))   # the stored inputs are the procedural ones
    assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    fps = F.fps_batch(x, S, start)
    new_xyz = np.stack([x[b, fps[b]] for b in range(B)])
    assert np.array_equal(_bits(new_xyz), _bits(GOLDEN[name + "_new_xyz"]))                            # every centre is a point of its cloud
    r2s = [G.r2_of(r) for r in radii]
    idx_cat, count = M.query_ball_msg_batch(x, new_xyz, r2s, nsamples)
    assert idx_cat.shape == (B, S, sum(nsamples)) and idx_cat.dtype == np.int64 and count.shape == (B, S, R) and count.dtype == np.int32
    assert (count >= 1).all()
    grouped = M.group_msg_batch(x, new_xyz, idx_cat, nsamples, pts)
    exact = all(r in G.EXACT_RADII for r in radii)
    for i, (view, off) in enumerate(zip(M.split(idx_cat, nsamples), M.offsets(nsamples))):
        want = GOLDEN["%s_idx%d" % (name, i)].astype(np.int64)
        assert np.array_equal(view, want) and np.array_equal(idx_cat[:, :, off:off + nsamples[i]], want), (name, i)
        want = GOLDEN["%s_grouped%d" % (name, i)]
        assert want.shape == (B, S, nsamples[i], D + 3) and want.dtype == F32
        assert np.array_equal(_bits(grouped[i]), _bits(want)), (name, i)
        assert (count[..., i] == nsamples[i]).any() and (count[..., i] < nsamples[i]).any()            # the cut and the padding, in every scale
        on_sphere = sum(int((np.take_along_axis(G.distances(new_xyz[b], x[b]), view[b], axis=1) == r2s[i]).any()) for b in range(B))
        if exact:
            assert float(r2s[i]) == radii[i] * radii[i] and on_sphere == B
            for b in range(B):
                assert M.planted_indices(start[b], R)[i] in view[b, 0]
        else:
            assert on_sphere == 0 and float(r2s[i]) * 2 ** 20 != round(float(r2s[i]) * 2 ** 20)


def test_golden_holds_both_cases_and_the_modules_state():
    assert {(c[4], c[5]) for c in M.GOLDEN_CASES.values()} == {((0.125, 0.25, 0.5), (4, 8, 16)), ((0.1, 0.2, 0.4), (8, 16, 32))}
    assert sorted(c[6] > 0 for c in M.GOLDEN_CASES.values()) == [False, True]                         # one D = 0, one D > 0
    for name, (seed, B, N, S, radii, nsamples, D, mlp_list) in M.GOLDEN_CASES.items():
        keys = [str(k) for k in GOLDEN[name + "_keys"]]
        assert [k for k in keys if k.startswith("conv_blocks.1.")][:2] == ["conv_blocks.1.0.weight", "conv_blocks.1.0.bias"]
        assert "bn_blocks.2.1.running_var" in keys and all((name + "_sd:" + k) in GOLDEN.files for k in keys)
        for mode in ("ev", "tr"):
            got = {k for k in GOLDEN.files if k.startswith("%s_%s_" % (name, mode))}
            assert ("%s_%s_dx:points" % (name, mode) in got) == (D > 0)
            assert "%s_%s_out:new_points" % (name, mode) in got and "%s_%s_d:bn_blocks.0.0.weight" % (name, mode) in got
            assert ("%s_%s_d:conv_blocks.0.0.bias" % (name, mode) in got) == (mode == "ev")            # zero in train mode: not recorded
        assert GOLDEN["%s_ev_out:new_points" % name].shape == (B, sum(m[-1] for m in mlp_list), S)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "msg.npz")) < 300 * 1024


def test_layout_repeated_radius_and_the_sum_order():
    x = np.zeros((10, 3), dtype=F32)
    x[:, 0] = [0.0, 5.0, 0.5, 1.0, 5.0, -1.0, 0.25, 5.0, 2.0, 1.0]
    c = np.array([[0, 0, 0], [5, 0, 0], [9, 9, 9]], dtype=F32)
    nsamples = (4, 2, 3)
    idx_cat, count = M.query_ball_msg(x, c, [F32(1.0), F32(0.25), F32(1.0)], nsamples)          # un-sorted, one radius twice
    assert M.offsets(nsamples) == [0, 4, 6]
    assert idx_cat[0].tolist() == [0, 2, 3, 5] + [0, 2] + [0, 2, 3] and count[0].tolist() == [4, 2, 3]
    assert idx_cat[1].tolist() == [1, 4, 7, 1] + [1, 4] + [1, 4, 7] and count[1].tolist() == [3, 2, 3]
    assert idx_cat[2].tolist() == [0] * 9 and count[2].tolist() == [0, 0, 0]                      # the empty group, in every scale
    assert np.array_equal(idx_cat[:, 6:9], idx_cat[:, 0:3])                                       # equal radii: the shorter list is a prefix
    pts = np.arange(20, dtype=F32).reshape(10, 2)
    outs = M.group_msg(x, c, idx_cat, nsamples, pts)
    assert [o.shape for o in outs] == [(3, 4, 5), (3, 2, 5), (3, 3, 5)]
    assert outs[0][0, :, :2].tolist() == [[0, 1], [4, 5], [6, 7], [10, 11]] and outs[0][0, :, 2].tolist() == [0.0, 0.5, 1.0, -1.0]   # attributes first
    assert outs[1][1, :, 2].tolist() == [0.0, 0.0] and [o.shape for o in M.group_msg(x, c, idx_cat, nsamples)] == [(3, 4, 3), (3, 2, 3), (3, 3, 3)]
    # the backward: point 0 is hit by centre 0 in scales 0, 1, 2 (edges 0, 4, 6) and by all nine slots of centre 2 (edges 18 .. 26);
    # with terms 2^24, 1, -2^24 first the order shows: ((2^24 + 1) - 2^24) = 0 in fp32, then the nine ones
    dgs = [np.zeros((3, k, 5), dtype=F32) for k in nsamples]
    dgs[0][0, 0, 0], dgs[1][0, 0, 0], dgs[2][0, 0, 0] = 2.0 ** 24, 1.0, -2.0 ** 24
    for g in dgs:
        g[2, :, 0] = 1.0
        g[:, :, 2:] = 77.0                                                                        # the coordinate columns go nowhere
    got = M.group_msg_bwd(dgs, idx_cat, nsamples, 10)
    assert got.shape == (10, 2) and got[0, 0] == 9.0 and got[0, 1] == 0.0 and got[8].tolist() == [0.0, 0.0]
    total, bound = M.group_msg_bwd_f64(dgs, idx_cat, nsamples, 10)
    assert total[0, 0] == 10.0 and abs(float(got[0, 0]) - total[0, 0]) <= bound[0, 0]
    terms = np.concatenate(dgs, axis=1).reshape(-1, 5)[:, :2].T
    assert np.array_equal(got, PG.ordered_sums(terms, *PG.reverse_lists(idx_cat, 10)).T)
    per, union = M.scanned_fraction(idx_cat, count, nsamples, 10)
    assert len(per) == 3 and all(0 < f <= 1 for f in per) and union >= max(per)


def test_header_binding_and_library_agree():
    from svnet_amd import _lib, group as Gr
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "svnet_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert _lib.DEFINES["SVNET_MSG_MAX_SCALES"] == 4 == Gr.MAX_SCALES
    S = _lib.SIGNATURES
    assert S["svnet_group_msg_supported"][1] == [_lib.c_i64, _lib.c_i64, _lib.c_i64, _lib.c_p, _lib.c_i64]
    assert len(S["svnet_ball_query_msg_f32"][1]) == 11 and S["svnet_ball_query_msg_f32"][1][5:8] == [_lib.c_i64, _lib.c_p, _lib.c_p]
    assert len(S["svnet_group_points_msg_f32"][1]) == 15 and len(S["svnet_group_points_msg_bwd_f32"][1]) == 14
    header_abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert L.svnet_version() == _lib.ABI_VERSION == header_abi and header_abi >= 427 and "427: svnet_ball_query_msg_f32" in header


def test_supported_query_and_refusals_without_a_gpu():
    from svnet_amd import _lib
    L = _lib.lib()

    def ns(*v):
        return (ctypes.c_int64 * len(v))(*v)

    for N, S, v, D in ((1, 1, (1,), 0), (32768, 1, (1, 32768, 5, 5), 0), (2048, 512, (16, 32, 128), 320)):
        assert L.svnet_group_msg_supported(N, S, len(v), ns(*v), D) == 1, (N, S, v, D)
    for N, S, v, D in ((5, 1, (6,), 0), (5, 1, (2, 6), 0), (5, 1, (2, 0), 0), (0, 1, (1,), 0), (32769, 1, (1,), 0), (5, 0, (1,), 0), (5, 1, (1,), -1)):
        assert L.svnet_group_msg_supported(N, S, len(v), ns(*v), D) == 0, (N, S, v, D)
    assert L.svnet_group_msg_supported(8, 4, 0, ns(1), 0) == 0 and L.svnet_group_msg_supported(8, 4, 5, ns(1, 1, 1, 1, 1), 0) == 0
    assert L.svnet_group_msg_supported(8, 4, 1, None, 0) == 0
    p = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused on the host
    r2, two = (ctypes.c_float * 4)(0.04, 0.04, 0.04, 0.04), ns(2, 3)
    q, g, w = L.svnet_ball_query_msg_f32, L.svnet_group_points_msg_f32, L.svnet_group_points_msg_bwd_f32
    assert q(None, p, 1, 8, 4, 2, r2, two, p, p, None) == -1 and b"null" in L.svnet_last_error()
    assert q(p, p, 1, 8, 4, 2, None, two, p, p, None) == -1 and q(p, p, 1, 8, 4, 2, r2, None, p, p, None) == -1
    assert q(p, p, 0, 8, 4, 2, r2, two, p, p, None) == -1 and b"positive" in L.svnet_last_error()
    assert q(p, p, 1, 8, 4, 0, r2, two, p, p, None) == -2 and b"scales" in L.svnet_last_error()
    assert q(p, p, 1, 8, 4, 5, r2, ns(1, 1, 1, 1, 1), p, p, None) == -2
    assert q(p, p, 1, 8, 4, 2, r2, ns(2, 9), p, p, None) == -2 and b"nsample" in L.svnet_last_error()
    assert q(p, p, 1, 32769, 4, 2, r2, two, p, p, None) == -2 and b"32768" in L.svnet_last_error()
    assert q(p, p, 1 << 29, 8, 4, 2, r2, two, p, p, None) == -2 and b"2^31" in L.svnet_last_error()
    assert g(p, None, p, p, 1, 8, 4, 2, two, 3, p, p, None, None, None) == -1 and b"null" in L.svnet_last_error()
    assert g(p, p, None, p, 1, 8, 4, 2, two, 3, p, p, None, None, None) == -1 and b"null points" in L.svnet_last_error()
    assert g(p, p, p, p, 1, 8, 4, 2, two, 3, p, None, None, None, None) == -1 and b"out1" in L.svnet_last_error()
    assert g(p, p, p, p, 0, 8, 4, 2, two, 3, p, p, None, None, None) == -1 and b"positive" in L.svnet_last_error()
    assert g(p, p, p, p, 1, 8, 4, 2, ns(2, 9), 3, p, p, None, None, None) == -2 and b"nsample" in L.svnet_last_error()
    assert g(p, p, p, p, 1, 8, 4, 2, two, -1, p, p, None, None, None) == -2
    assert g(p, p, p, p, 1 << 29, 8, 4, 2, two, 3, p, p, None, None, None) == -2 and b"2^31" in L.svnet_last_error()
    assert w(p, None, None, None, p, p, 1, 8, 4, 2, two, 3, p, None) == -1 and b"dg1" in L.svnet_last_error()
    assert w(p, p, None, None, None, p, 1, 8, 4, 2, two, 3, p, None) == -1 and b"null" in L.svnet_last_error()
    assert w(p, p, None, None, p, p, 1, 8, 4, 2, two, 0, p, None) == -2 and b"D >= 1" in L.svnet_last_error()
    assert w(p, p, None, None, p, p, 1, 8, 4, 5, ns(1, 1, 1, 1, 1), 3, p, None) == -2
    assert w(p, p, None, None, p, p, 1 << 29, 8, 4, 2, two, 3, p, None) == -2 and b"2^31" in L.svnet_last_error()


def test_argument_validation_without_a_gpu():
    from svnet_amd import group as Gr
    x, c, pts = (torch.from_numpy(a) for a in G.lattice_case(43, 2, 10, 5, 4))
    idx = torch.zeros(2, 5, 5, dtype=torch.int64)
    dgs = [torch.zeros(2, 5, 2, 7), torch.zeros(2, 5, 3, 7)]
    for call in (lambda: Gr.query_ball_point_msg((0.2, 0.4), (2, 3), x, c), lambda: Gr.group_points_msg(x, c, idx, (2, 3), pts),
                 lambda: Gr.group_points_msg(x, c, idx, (2, 3)), lambda: Gr.sample_and_group_msg(5, (0.2, 0.4), (2, 3), x, pts),
                 lambda: Gr.group_points_msg_backward(dgs, idx, (2, 3), 10),
                 lambda: Gr.query_ball_point_msg((0.2, 0.4), (2, 11), x, c)):        # nsample_i > N is the library's refusal, behind the device's
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="2 radii for 3 nsample"):                    # list length mismatch
        Gr.query_ball_point_msg((0.2, 0.4), (2, 3, 4), x, c)
    with pytest.raises(ValueError, match="radii"):
        Gr.sample_and_group_msg(5, (0.2,), (2, 3), x, pts)
    with pytest.raises(ValueError, match="0 scales"):
        Gr.query_ball_point_msg((), (), x, c)
    with pytest.raises(ValueError, match="5 scales"):
        Gr.query_ball_point_msg((0.1,) * 5, (1,) * 5, x, c)
    with pytest.raises(ValueError, match="5 scales"):
        Gr.group_points_msg(x, c, idx, (1,) * 5, pts)
    with pytest.raises(ValueError, match="0 scales"):
        Gr.sample_and_group_msg(5, (), (), x, pts)
    with pytest.raises(ValueError, match="gradients for"):
        Gr.group_points_msg_backward(dgs[:1], idx, (2, 3), 10)
    with pytest.raises(ValueError):
        Gr.group_points_msg(x, c, idx, (2, 2), pts)                         # Ktot differs from idx_cat's
    with pytest.raises(ValueError):
        Gr.group_points_msg_backward([dgs[0], dgs[0]], idx, (2, 3), 10)     # a gradient of the wrong nsample
    with pytest.raises(ValueError):
        Gr.split_scales(idx, (2, 2))
    assert [tuple(v.shape) for v in Gr.split_scales(idx, (2, 3))] == [(2, 5, 2), (2, 5, 3)]
    with pytest.raises(TypeError):
        Gr.query_ball_point_msg((0.2,), (3,), x.numpy(), c)
    with pytest.raises(TypeError):
        Gr.query_ball_point_msg((0.2,), (3,), x.double(), c)
    with pytest.raises(TypeError):
        Gr.group_points_msg(x, c, idx.int(), (2, 3), pts)
    with pytest.raises(TypeError):
        Gr.group_points_msg(x, c, idx, (2, 3), pts.half())
    with pytest.raises(TypeError):
        Gr.sample_and_group_msg(5, (0.2,), (3,), x, pts, start=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        Gr.group_points_msg_backward([dgs[0].double(), dgs[1]], idx, (2, 3), 10)
    with pytest.raises(ValueError, match="contiguous"):
        Gr.query_ball_point_msg((0.2,), (3,), x.permute(1, 0, 2), c)
    with pytest.raises(ValueError, match="contiguous"):
        Gr.group_points_msg(x, c, torch.zeros(2, 5, 10, dtype=torch.int64)[:, :, ::2], (2, 3), pts)
    with pytest.raises(ValueError):
        Gr.query_ball_point_msg((0.2,), (3,), x, c[:1])                     # batch mismatch
    with pytest.raises(ValueError):
        Gr.group_points_msg(x, c, idx, (2, 3), pts[:, :9].contiguous())     # points' N differs from xyz's
    with pytest.raises(ValueError, match="forward only"):
        Gr.query_ball_point_msg((0.2,), (3,), x.clone().requires_grad_(), c)
    with pytest.raises(ValueError, match="forward only"):
        Gr.group_points_msg(x, c.clone().requires_grad_(), idx, (2, 3), pts)
    with pytest.raises(ValueError, match="forward only"):
        Gr.sample_and_group_msg(5, (0.2,), (3,), x.clone().requires_grad_(), pts)
    with pytest.raises(ValueError, match="forward only"):
        Gr.group_points_msg(x, c, idx, (2, 3), pts.clone().requires_grad_())         # off a HIP device the grouping is forward only
    with pytest.raises(ValueError):
        Gr.group_points_msg(x, c, idx, (2, 3), pts.to("meta"))              # mismatched devices


def test_module_has_the_references_keys_and_signature():
    from svnet_amd.models.utils import pointnet_msg as U, pointnet_util
    assert "PointNetSetAbstractionMsg" in U.__all__ and "is not here" not in pointnet_util.__doc__ and "pointnet_msg.py" in pointnet_util.__doc__
    assert list(inspect.signature(U.PointNetSetAbstractionMsg.__init__).parameters)[1:] == ["npoint", "radius_list", "nsample_list", "in_channel", "mlp_list"]
    assert list(inspect.signature(U.PointNetSetAbstractionMsg.forward).parameters)[1:] == ["xyz", "points", "start"]
    for name, (seed, B, N, S, radii, nsamples, D, mlp_list) in M.GOLDEN_CASES.items():
        mod = U.PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlp_list])
        keys = [str(k) for k in GOLDEN[name + "_keys"]]
        shapes = [tuple(int(v) for v in row if v >= 0) for row in GOLDEN[name + "_shapes"]]
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == list(zip(keys, shapes))
        state = {k: torch.from_numpy(GOLDEN["%s_sd:%s" % (name, k)]) for k in keys}
        mod.load_state_dict(state, strict=True)
        assert all(torch.equal(v, state[k]) for k, v in mod.state_dict().items())
        assert isinstance(mod.conv_blocks[0][0], torch.nn.Conv2d) and isinstance(mod.bn_blocks[0][0], torch.nn.BatchNorm2d)
        assert mod.seed == 0
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(torch.zeros(B, 3, N), None if D == 0 else torch.zeros(B, D, N))
