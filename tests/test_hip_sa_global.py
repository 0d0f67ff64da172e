"""GPU tests (-m gpu) of the fused global set-abstraction level: svnet_sa_global_f32 (svnet_amd/csrc/sa_global.hip) through
svnet_amd.sa_global, against the numpy restatement tests/sa_global_ref.py, the existing fused kernel where both admit the level, the
module's own eval forward and the reference's recorded outputs (tests/golden/sa_global.npz).  The contract is a fixed fmaf chain per
output and an order-free maximum, so the kernel's results are compared as BIT PATTERNS (a -0 counted as +0); the wrapper against the
module, which rounds differently, within the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every case runs at
B = 2; every reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import sa_fused_ref as R
from tests import sa_global_ref as SG
from tests.common import compare_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "sa_global.npz"))
F32 = np.float32
B = 2
_once = FL.cache()

# (N, D, widths): every N in {1, 15, 16, 17, 47, 49, 64, 65, 131} (below, at and past one 16-row MFMA tile, three tiles less and more
# than a point, one workgroup's 64 rows and one more, three workgroups), every C0 = 3 + D in {3, 4, 7, 67, 134} (K of the first product
# below, at and past one k-step, a multiple of nothing), one to four layers, widths that are no multiple of the 16-column tile, 196
# (more column tiles than waves), 257 and 300 (past the 256 of the other fused kernels), and the classifier's own widths once.
CASES = [(1, 0, (5,)),
         (15, 1, (12, 20)),
         (16, 4, (33, 8, 196)),
         (17, 64, (16, 16, 16, 7)),
         (47, 131, (257,)),
         (49, 0, (8, 300)),
         (64, 1, (5,)),
         (65, 4, (12, 20)),
         (131, 64, (33, 8, 196)),
         (131, 131, (8, 300)),
         (33, 0, (256, 512, 1024))]
# One case per row plan with N = rows + 1, so that two workgroups share a cloud and the second holds one row.  D and the widths follow
# from the header's formula, 4 R (stride0 + stride1) + 4 pad16(C_L) <= 163840 (worked out in tests/test_host_sa_global.py):
# (rows, N, D, widths)
CROSSING = [(64, 65, 0, (5,)), (48, 49, 700, (8,)), (32, 33, 1000, (8,)), (16, 17, 1000, (600, 8))]


def _inputs(N, D, positive=False):
    """(xyz [B,3,N], points [B,D,N] or None), channel-first."""
    def make():
        x = (synth.normal(7000 + N, 1, (B, 3, N)) * F32(0.5)).astype(F32)
        pts = synth.normal(7000 + N, 2 + D, (B, D, N)) if D else None
        if positive:
            x, pts = np.abs(x) + F32(0.125), None if pts is None else np.abs(pts) + F32(0.125)
        return x, pts
    return _once(("in", N, D, positive), make)


def _want(N, D, widths):
    def make():
        x, pts = _inputs(N, D)
        return SG.level_batch(x, pts, FL.state(9100 + D, 3 + D, widths)[1])
    return _once(("want", N, D, widths), make)


@pytest.mark.parametrize("N,D,widths", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_global_level_equals_the_restatement_bit_for_bit(N, D, widths, hip_device):
    from svnet_amd import sa_fused as SF
    from svnet_amd import sa_global as SGL
    dev = hip_device
    x, pts = _inputs(N, D)
    want = _want(N, D, widths)
    level, _ = FL.level(dev, 9100 + D, 3 + D, widths)
    tag = "N %d D %d widths %s" % (N, D, widths)
    tx, tp = FL.dev(dev, x, pts)
    got = SGL.global_mlp_max(tx, tp, level)
    C = widths[-1]
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, C, 1) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert float(want.max()) > 0
    FL.same_bits(SGL.global_mlp_max(tx, tp, level), want, tag + ", again")
    # into channels 3 .. of a NaN-filled [B,C_total,1]: the other channels stay NaN
    buf = torch.full((B, C + 5, 1), float("nan"), dtype=torch.float32, device=dev)
    assert SGL.global_mlp_max(tx, tp, level, out=buf, c_off=3) is buf
    FL.same_bits(buf[:, 3:3 + C].contiguous(), want, tag + ", c_off 3")
    assert torch.isnan(buf[:, :3]).all() and torch.isnan(buf[:, 3 + C:]).all()
    # one cloud on its own (B 1) has the bits it has inside the batch
    alone = SGL.global_mlp_max(tx[B - 1:], None if tp is None else tp[B - 1:], level)
    FL.same_bits(alone, want[B - 1:], tag + ", one cloud alone")
    # a maximum has no order: the points of a cloud permuted
    perm = torch.from_numpy(np.argsort(synth.integers(78, N, (N,), 1 << 30), kind="stable")).to(dev)
    FL.same_bits(SGL.global_mlp_max(tx[:, :, perm].contiguous(), None if tp is None else tp[:, :, perm].contiguous(), level), want, tag + ", points permuted")
    # where the existing fused kernel admits the level too: one centre at 0 whose group is all points in order
    assert SF.supported(N, 1, N, D, widths) == (max(widths) <= 256)
    if max(widths) <= 256:
        idx = torch.arange(N, dtype=torch.int64, device=dev).view(1, 1, N).expand(B, 1, N).contiguous()
        rows = tx.permute(0, 2, 1).contiguous()
        attrs = None if tp is None else tp.permute(0, 2, 1).contiguous()
        other = SF.group_mlp_max(rows, torch.zeros(B, 1, 3, dtype=torch.float32, device=dev), idx, attrs, level)
        assert torch.equal(other.view(torch.int32), got.view(torch.int32)), tag + ", against sa_fused_kernel"


@pytest.mark.parametrize("rows,N,D,widths", CROSSING, ids=lambda v: str(v).replace(" ", ""))
def test_two_workgroups_share_a_cloud_at_every_row_plan(rows, N, D, widths, hip_device):
    from svnet_amd import sa_global as SGL
    dev = hip_device
    assert SGL.rows_tile(D, widths) == rows and N == rows + 1
    x, pts = _inputs(N, D)
    want = _want(N, D, widths)
    level, _ = FL.level(dev, 9100 + D, 3 + D, widths)
    tx, tp = FL.dev(dev, x, pts)
    tag = "rows %d N %d D %d widths %s" % (rows, N, D, widths)
    FL.same_bits(SGL.global_mlp_max(tx, tp, level), want, tag)
    assert float(want.max()) > 0
    # the first tile on its own: one workgroup per cloud
    head = SG.level_batch(x[:, :, :rows], None if pts is None else pts[:, :, :rows], FL.state(9100 + D, 3 + D, widths)[1])
    assert (head <= want).all()
    FL.same_bits(SGL.global_mlp_max(tx[:, :, :rows].contiguous(), None if tp is None else tp[:, :, :rows].contiguous(), level), head, tag + ", one tile")


@pytest.mark.parametrize("where", ["first_tile", "last_partial_tile"])
def test_the_maximum_is_found_wherever_it_lies(where, hip_device):
    """N 131 is two tiles of 64 rows and one of 3.  All points are small but one, planted at row 5 or at row 130; the restatement
    says that the planted row alone holds the maximum of more than a quarter of the columns."""
    from svnet_amd import sa_global as SGL
    dev = hip_device
    N, D, widths = 131, 4, (12, 20)
    p = 5 if where == "first_tile" else N - 1
    assert SGL.rows_tile(D, widths) == 64 and N - 1 >= 128

    def make():
        x, pts = (a.copy() for a in _inputs(N, D))
        x, pts = (x * F32(2.0 ** -6)).astype(F32), (pts * F32(2.0 ** -6)).astype(F32)
        x[:, :, p], pts[:, :, p] = _inputs(N, D)[0][:, :, p] * F32(8), _inputs(N, D)[1][:, :, p] * F32(8)
        layers = FL.state(9100 + D, 3 + D, widths)[1]
        h = R.mlp(np.concatenate([x, pts], axis=1).transpose(0, 2, 1), layers)                  # [B,N,C]
        rest = np.delete(h, p, axis=1).max(axis=1)
        return x, pts, SG.level_batch(x, pts, layers), (h[:, p] > rest).mean()
    x, pts, want, share = _once(("planted", where), make)
    assert share > 0.25, share
    level, _ = FL.level(dev, 9100 + D, 3 + D, widths)
    tx, tp = FL.dev(dev, x, pts)
    FL.same_bits(SGL.global_mlp_max(tx, tp, level), want, where)


def test_rows_past_the_cloud_never_enter_the_maximum(hip_device):
    """N 17: the second 16-row tile holds one real row and fifteen zero rows.  The last layer's folded bias is 8 and its weights are
    negative on positive inputs: a zero row gives exactly 8 and would beat every real row."""
    from svnet_amd import sa_global as SGL
    dev = hip_device
    N, D, widths = 17, 4, (8,)
    x, pts = _inputs(N, D, positive=True)
    level, folded = FL.level(dev, 41, 3 + D, widths, kind="padding")
    assert (folded[-1][0] < 0).all() and (folded[-1][1] == F32(8)).all() and x.min() > 0 and pts.min() > 0
    want = _once(("padding",), lambda: SG.level_batch(x, pts, folded))
    assert (want < 8).all() and (want > 0).all()
    tx, tp = FL.dev(dev, x, pts)
    FL.same_bits(SGL.global_mlp_max(tx, tp, level), want, "padding rows")


def test_a_level_whose_last_layer_is_negative_everywhere_gives_exact_zeros(hip_device):
    from svnet_amd import sa_global as SGL
    dev = hip_device
    N, D, widths = 65, 1, (12, 20)
    x, pts = _inputs(N, D)
    level, folded = FL.level(dev, 31, 3 + D, widths, kind="negative_last")
    assert (folded[-1][1] < 0).all() and not folded[-1][0].any()
    tx, tp = FL.dev(dev, x, pts)
    got = SGL.global_mlp_max(tx, tp, level, out=torch.full((B, widths[-1], 1), float("nan"), dtype=torch.float32, device=dev))
    assert not FL.bits(got).any()


def test_a_second_call_into_the_same_buffer_leaves_no_stale_maxima(hip_device):
    """Positive weights on positive inputs: halving the inputs makes every output smaller.  The second call into the same buffer
    must give the second result - an integer maximum into a buffer that was not set to +0 first would keep the first."""
    from svnet_amd import sa_global as SGL
    dev = hip_device
    N, D, widths = 65, 4, (20,)
    x, pts = _inputs(N, D, positive=True)
    level, folded = FL.level(dev, 43, 3 + D, widths, kind="positive")
    x2, pts2 = (x * F32(0.5)).astype(F32), (pts * F32(0.5)).astype(F32)
    want1, want2 = _once(("stale",), lambda: (SG.level_batch(x, pts, folded), SG.level_batch(x2, pts2, folded)))
    assert (want2 < want1).all() and (want2 > 0).all()
    buf = torch.empty(B, widths[-1], 1, dtype=torch.float32, device=dev)
    FL.same_bits(SGL.global_mlp_max(*FL.dev(dev, x, pts), level, out=buf), want1, "first call")
    FL.same_bits(SGL.global_mlp_max(*FL.dev(dev, x2, pts2), level, out=buf), want2, "second call")


# ---- the wrapper
def _golden_module(dev):
    """(module in eval mode on the device, xyz [B,3,N], points [B,D,N], the recorded outputs)."""
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    seed, Bc, N, D, mlp = SG.GOLDEN_CASE
    mod = PointNetSetAbstraction(None, None, None, D + 3, list(mlp), True)
    mod.load_state_dict({str(k): torch.from_numpy(GOLDEN["sd:" + str(k)]) for k in GOLDEN["keys"]}, strict=True)
    xyz, points = FL.dev(dev, GOLDEN["xyz"], GOLDEN["points"])
    return mod.to(dev).eval(), xyz, points, {"out:new_xyz": GOLDEN["ev_out:new_xyz"], "out:new_points": GOLDEN["ev_out:new_points"]}


def test_wrapper_equals_the_module_and_the_recorded_reference(hip_device):
    """FusedGlobalAbstraction against the module's own eval forward on the same state_dict and against the reference's recorded eval
    outputs, both within compare_case(..., 1e-3); against the restatement bit for bit; new_xyz exact zeros [B,3,1].  Then refresh()."""
    from svnet_amd import sa_global as SGL
    seed, Bc, N, D, mlp = SG.GOLDEN_CASE
    mod, xyz, points, ref = _golden_module(hip_device)
    fused = SGL.FusedGlobalAbstraction(mod)
    assert fused.supported(N, D) and not fused.supported(N, D + 1)
    new_xyz, new_points = fused(xyz, points, start=torch.zeros(Bc, dtype=torch.int64, device=hip_device))
    with torch.no_grad():
        mod_xyz, mod_points = mod(xyz, points)
    assert new_points.dtype == torch.float32 and new_points.shape == mod_points.shape == (Bc, mlp[-1], 1) and not new_points.requires_grad
    assert tuple(new_xyz.shape) == (Bc, 3, 1) and new_xyz.dtype == torch.float32 and not new_xyz.view(torch.int32).any() and torch.equal(new_xyz, mod_xyz)
    got = {"out:new_xyz": new_xyz.cpu().numpy(), "out:new_points": new_points.cpu().numpy()}
    worst_mod = compare_case(got, {"out:new_xyz": mod_xyz.cpu().numpy(), "out:new_points": mod_points.cpu().numpy()}, 1e-3, "against the module")
    worst_ref = compare_case(got, ref, 1e-3, "against the recorded reference")
    print("worst relative error %.3e against the module, %.3e against the reference" % (worst_mod[0], worst_ref[0]))
    state = {str(k): GOLDEN["sd:" + str(k)] for k in GOLDEN["keys"]}
    FL.same_bits(new_points, SG.level_batch(GOLDEN["xyz"], GOLDEN["points"], R.fold_state(state, R.single_prefixes(len(mlp)))), "the wrapper")
    # views, as a model hands them over, are taken
    wide = torch.cat([xyz, points], dim=1)
    again = fused(wide[:, :3], wide[:, 3:])[1]
    assert torch.equal(again.view(torch.int32), new_points.view(torch.int32))
    # new running statistics: stale until refresh()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.add_(0.25)
        moved = mod(xyz, points)[1]
    assert torch.equal(fused(xyz, points)[1].view(torch.int32), new_points.view(torch.int32))
    fresh = fused.refresh()(xyz, points)[1]
    compare_case({"out:new_points": fresh.cpu().numpy()}, {"out:new_points": moved.cpu().numpy()}, 1e-3, "refreshed")
    assert not torch.equal(fresh, new_points)


def test_wrapper_refuses_train_mode_and_falls_back_outside_the_envelope(hip_device):
    from svnet_amd import sa_global as SGL
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    dev = hip_device
    mod, xyz, points, _ = _golden_module(dev)
    fused = SGL.FusedGlobalAbstraction(mod)
    mod.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(xyz, points)
    mod.eval()
    with pytest.raises(ValueError, match="xyz requires grad"):
        fused(xyz.clone().requires_grad_(), points)
    # a layer of 1100 channels is outside the kernel's limits: the module's own forward, bit for bit
    torch.manual_seed(5)
    wide = PointNetSetAbstraction(None, None, None, 3, [16, 1100], True).to(dev).eval()
    fused = SGL.FusedGlobalAbstraction(wide)
    x = FL.dev(dev, _inputs(49, 0)[0])[0]
    assert not fused.supported(49, 0)
    got, want = fused(x, None), wide(x, None)
    assert tuple(got[1].shape) == (B, 1100, 1) and not got[1].requires_grad
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].detach().view(torch.int32))
    level = fused.level
    with pytest.raises(RuntimeError, match="not supported"):
        SGL.global_mlp_max(x, None, level)


def test_wrapper_in_a_captured_graph(hip_device):
    """The wrapper captured on a side stream after a warm-up; two replays with the inputs refilled in place between them each give the
    eager result bit for bit."""
    from svnet_amd import sa_global as SGL
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    dev = hip_device
    N, D = 131, 5
    torch.manual_seed(9)
    mod = PointNetSetAbstraction(None, None, None, D + 3, [12, 20, 260], True).to(dev).eval()
    fused = SGL.FusedGlobalAbstraction(mod)
    sets = []
    for seed in (90, 91):
        sets.append(FL.dev(dev, synth.normal(seed, 1, (B, 3, N)) * F32(0.5), synth.normal(seed, 2, (B, D, N))))
    x, pts = (t.clone() for t in sets[0])

    def run():
        return fused(x, pts)

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = run()
    for s in (sets[1], sets[0]):
        for dst, src in zip((x, pts), s):
            dst.copy_(src)
        res[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = [r.clone() for r in res]
        eager = run()
        for a, b in zip(replayed, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.isnan(a).any()
        compare_case({"out:new_points": replayed[1].cpu().numpy()}, {"out:new_points": mod(x, pts)[1].detach().cpu().numpy()}, 1e-3,
                     "captured against the module")
