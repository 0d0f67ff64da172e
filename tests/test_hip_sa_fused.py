"""GPU tests (-m gpu) of the fused set-abstraction level: svnet_sa_fold_f32 and svnet_sa_fused_f32 (svnet_amd/csrc/sa_fused.hip)
through svnet_amd.sa_fused, against the numpy restatement tests/sa_fused_ref.py, the modules' own eval forward and the reference's
recorded outputs (tests/golden/msg.npz, tests/golden/sa_fused.npz).  The contract is a fixed fmaf chain per output and an order-free
maximum, so the kernel's results are compared as BIT PATTERNS (a -0 counted as +0); the wrapper against the modules, which round
differently, within the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every case runs at B = 2; every
reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import group_ref as G
from tests import msg_ref as M
from tests import sa_fused_ref as R
from tests.common import compare_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MSG = np.load(os.path.join(HERE, "golden", "msg.npz"))
GOLDEN = np.load(os.path.join(HERE, "golden", "sa_fused.npz"))
F32 = np.float32
B = 2
_once = FL.cache()


def _tile():
    try:
        from svnet_amd import sa_fused as SF
        return SF.rows_tile()
    except Exception:                 # the library or the module is missing: the tests still fail, at the import in the test
        return 64


T = _tile()
# (N, S, K, D, widths): every K in {1, 2, tile - 1, tile, tile + 1, 2 tile + 3} (whole centres sharing a tile, one centre filling it,
# one centre over two and three tiles), every S in {1, 3, 5, 33} (partial workgroups), every C0 = 3 + D in {3, 4, 7, 67, 131} (K of the
# first product below, at and past one k-step, a multiple of nothing), one to four layers, widths that are no multiple of the 16-column
# tile, 196 and 256 (more column tiles than waves).  The last two are the shapes of real levels in small: two centres per tile and
# eight column tiles; sixteen column tiles, four per wave.
CASES = [(1, 1, 1, 0, (5,)),
         (40, 3, 2, 1, (12, 20)),
         (200, 5, T - 1, 4, (33, 8, 196)),
         (200, 33, T, 64, (16, 16, 16, 7)),
         (300, 3, T + 1, 128, (12, 20)),
         (300, 5, 2 * T + 3, 0, (33, 8, 196)),
         (128, 33, 32, 0, (64, 64, 128)),
         (64, 5, 16, 3, (256,))]


def _inputs(N, S, K, D):
    def make():
        x, c, pts = G.gauss_case(8000 + N + S, B, N, S, D)
        idx = synth.integers(8100 + N, S, (B, S, K), N).astype(np.int64)
        idx[:, :, 0], idx[:, :, -1] = -7, N + 3                              # outside the cloud: clamped, never followed
        return x, np.ascontiguousarray(c), pts, idx
    return _once(("in", N, S, K, D), make)


def _want(N, S, K, D, widths, xyz_last):
    def make():
        x, c, pts, idx = _inputs(N, S, K, D)
        return R.level_batch(x, c, idx, pts, FL.state(9000 + 3 + D, 3 + D, widths)[1], xyz_last)
    return _once(("want", N, S, K, D, widths, xyz_last), make)


def test_fold_equals_the_restatement_bit_for_bit(hip_device):
    """Wf and bf of every layer (the comparison is in fused_level_cases.level), widths 1 .. 256 and inputs 1 .. 324 that are multiples of nothing;
    refresh() after the statistics changed folds the new ones."""
    for seed, C0, widths in [(1, 3, (5,)), (2, 324, (256, 1, 196)), (3, 131, (16, 16, 16, 7)), (4, 1, (3,))]:
        FL.level(hip_device, seed, C0, widths)
    level, folded = FL.level(hip_device, 5, 7, (12, 20))
    state = FL.state(5, 7, (12, 20))[0]
    with torch.no_grad():
        level.bns[1].running_var.mul_(3.0)
    level.refresh()
    Wf, bf = R.fold(state[1]["W"], state[1]["b"], state[1]["gamma"], state[1]["beta"], state[1]["mean"], state[1]["var"] * F32(3.0), 1e-5)
    assert np.array_equal(level.wf[1].cpu().numpy().view(np.uint32), Wf.view(np.uint32)) and not np.array_equal(Wf, folded[1][0])
    assert np.array_equal(level.bf[1].cpu().numpy().view(np.uint32), bf.view(np.uint32))
    assert np.array_equal(level.wf[0].cpu().numpy().view(np.uint32), folded[0][0].view(np.uint32))


@pytest.mark.parametrize("xyz_last", [False, True], ids=["xyz_first", "xyz_last"])
@pytest.mark.parametrize("N,S,K,D,widths", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_level_equals_the_restatement_bit_for_bit(N, S, K, D, widths, xyz_last, hip_device):
    from svnet_amd import sa_fused as SF
    dev = hip_device
    x, c, pts, idx = _inputs(N, S, K, D)
    want = _want(N, S, K, D, widths, xyz_last)
    level, _ = FL.level(dev, 9000 + 3 + D, 3 + D, widths)
    tag = "N %d S %d K %d D %d widths %s xyz_last %s" % (N, S, K, D, widths, xyz_last)
    tx, tc, tp, ti = FL.dev(dev, x, c, pts, idx)
    got = SF.group_mlp_max(tx, tc, ti, tp, level, xyz_last=xyz_last)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, widths[-1], S) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert float(want.max()) > 0
    # a second run; the indices as columns 3 .. 3 + K - 1 of a wider table (idx_ld = K + 5)
    FL.same_bits(SF.group_mlp_max(tx, tc, ti, tp, level, xyz_last=xyz_last), want, tag + ", again")
    wide = torch.full((B, S, K + 5), N + 11, dtype=torch.int64, device=dev)
    wide[:, :, 3:3 + K] = ti
    view = wide[:, :, 3:3 + K]
    assert not view.is_contiguous() or S == 1
    FL.same_bits(SF.group_mlp_max(tx, tc, view, tp, level, xyz_last=xyz_last), want, tag + ", idx_ld > K")
    # into channels 3 .. of a NaN-filled [B,C_total,S]: the other channels stay NaN
    C = widths[-1]
    buf = torch.full((B, C + 5, S), float("nan"), dtype=torch.float32, device=dev)
    assert SF.group_mlp_max(tx, tc, ti, tp, level, xyz_last=xyz_last, out=buf, c_off=3) is buf
    FL.same_bits(buf[:, 3:3 + C].contiguous(), want, tag + ", c_off 3")
    assert torch.isnan(buf[:, :3]).all() and torch.isnan(buf[:, 3 + C:]).all()
    # permuting the slots of every group changes nothing: a maximum has no order
    perm = torch.from_numpy(np.argsort(synth.integers(77, K, (K,), 1 << 30), kind="stable")).to(dev)
    FL.same_bits(SF.group_mlp_max(tx, tc, ti[:, :, perm].contiguous(), tp, level, xyz_last=xyz_last), want, tag + ", slots permuted")
    # one centre on its own (B 1, S 1) has the bits it has inside the batch
    b, s = B - 1, S // 2
    alone = SF.group_mlp_max(tx[b:b + 1], tc[b:b + 1, s:s + 1].contiguous(), ti[b:b + 1, s:s + 1].contiguous(), None if tp is None else tp[b:b + 1],
                             level, xyz_last=xyz_last)
    FL.same_bits(alone, want[b:b + 1, :, s:s + 1], tag + ", one centre alone")


# (N, S, radius, K, D, widths): groups from the query's restatement - full, padded and (centre 1, planted far away) empty ones - below,
# at and above one tile of rows
COUNT_CASES = [(150, 5, 0.4, 16, 2, (12, 20)), (300, 3, 0.6, T, 0, (33, 8)), (400, 5, 0.9, 2 * T + 3, 1, (16, 7))]


@pytest.mark.parametrize("N,S,radius,K,D,widths", COUNT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_padded_and_empty_groups_with_and_without_count(N, S, radius, K, D, widths, hip_device):
    from svnet_amd import sa_fused as SF
    dev = hip_device

    def make():
        x, c, pts = G.gauss_case(8300 + N, B, N, S, D)
        c = np.ascontiguousarray(c)
        c[:, 1] = 9.0                                                        # no point within the radius: the empty group
        idx, count = G.query_ball_batch(x, c, G.r2_of(radius), K)
        return x, c, pts, idx, count, R.level_batch(x, c, idx, pts, FL.state(8300 + K, 3 + D, widths)[1])
    x, c, pts, idx, count, want = _once(("count", N, S, radius, K, D, widths), make)
    assert (count[:, 1] == 0).all() and (idx[:, 1] == 0).all() and (count < K).any() and (count[:, 0] >= 1).all()
    level, _ = FL.level(dev, 8300 + K, 3 + D, widths)
    tx, tc, tp, ti, tn = FL.dev(dev, x, c, pts, idx, count)
    tag = "N %d S %d K %d D %d" % (N, S, K, D)
    FL.same_bits(SF.group_mlp_max(tx, tc, ti, tp, level), want, tag + ", all slots")
    FL.same_bits(SF.group_mlp_max(tx, tc, ti, tp, level, count=tn), want, tag + ", with count")
    # count as a column of a [B,S,3] table (count_ld = 3), and the slots past count overwritten: with count they are never read
    table = torch.full((B, S, 3), K, dtype=torch.int32, device=dev)
    table[:, :, 1] = tn
    junk = ti.clone()
    slot = torch.arange(K, device=dev).view(1, 1, K)
    junk[slot.expand(B, S, K) >= tn.clamp(min=1).unsqueeze(2)] = N // 2
    FL.same_bits(SF.group_mlp_max(tx, tc, junk, tp, level, count=table[:, :, 1]), want, tag + ", count_ld 3, junk past count")


def test_a_level_whose_last_layer_is_negative_everywhere_gives_exact_zeros(hip_device):
    from svnet_amd import sa_fused as SF
    dev = hip_device
    N, S, K, D, widths = 128, 33, 32, 0, (64, 64, 128)
    x, c, pts, idx = _inputs(N, S, K, D)
    level, folded = FL.level(dev, 31, 3, widths, kind="negative_last")
    assert (folded[-1][1] < 0).all() and not folded[-1][0].any()
    tx, tc, ti = FL.dev(dev, x, c, idx)
    got = SF.group_mlp_max(tx, tc, ti, None, level, out=torch.full((B, widths[-1], S), float("nan"), dtype=torch.float32, device=dev))
    assert not FL.bits(got).any()


# ---- the wrapper
def _golden_module(name, dev):
    """(module in eval mode on the device, xyz [B,3,N], points [B,D,N] or None, start, the recorded new_xyz [B,3,S] and new_points)."""
    if name == "single":
        from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
        seed, Bc, N, S, radius, nsample, D, mlp = R.GOLDEN_CASE
        mod = PointNetSetAbstraction(S, radius, nsample, D + 3, list(mlp), False)
        mod.load_state_dict({str(k): torch.from_numpy(GOLDEN["sd:" + str(k)]) for k in GOLDEN["keys"]}, strict=True)
        x, pts, start = GOLDEN["xyz"], GOLDEN["points"], GOLDEN["start"]
        ref = {"out:new_xyz": GOLDEN["ev_out:new_xyz"], "out:new_points": GOLDEN["ev_out:new_points"]}
    else:
        from svnet_amd.models.utils.pointnet_msg import PointNetSetAbstractionMsg
        seed, Bc, N, S, radii, nsamples, D, mlp_list = M.GOLDEN_CASES[name]
        mod = PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlp_list])
        mod.load_state_dict({str(k): torch.from_numpy(MSG["%s_sd:%s" % (name, k)]) for k in MSG[name + "_keys"]}, strict=True)
        x, pts, start = MSG[name + "_xyz"], MSG[name + "_points"] if D else None, MSG[name + "_start"]
        ref = {"out:new_xyz": MSG[name + "_ev_out:new_xyz"], "out:new_points": MSG[name + "_ev_out:new_points"]}
    xyz, points, start = FL.dev(dev, x.transpose(0, 2, 1), None if pts is None else pts.transpose(0, 2, 1), start)
    return mod.to(dev).eval(), xyz, points, start, ref


@pytest.mark.parametrize("name", ["single"] + list(M.GOLDEN_CASES))
def test_wrapper_equals_the_module_and_the_recorded_reference(name, hip_device):
    """FusedSetAbstraction against the module's own eval forward on the same state_dict and against the reference's recorded eval
    outputs, both within compare_case(..., 1e-3), the project's activation tolerance (the composed path rounds the BatchNorm after the
    convolution, the fused one folds it in); the sampled centres bit for bit.  Then the default start, and refresh()."""
    from svnet_amd import sa_fused as SF
    mod, xyz, points, start, ref = _golden_module(name, hip_device)
    fused = SF.FusedSetAbstraction(mod)
    new_xyz, new_points = fused(xyz, points, start=start)
    with torch.no_grad():
        mod_xyz, mod_points = mod(xyz, points, start=start)
    assert new_points.dtype == torch.float32 and new_points.shape == mod_points.shape and not new_points.requires_grad
    assert torch.equal(new_xyz.view(torch.int32), mod_xyz.view(torch.int32)) and new_xyz.shape == mod_xyz.shape
    got = {"out:new_xyz": new_xyz.cpu().numpy(), "out:new_points": new_points.cpu().numpy()}
    worst_mod = compare_case(got, {"out:new_xyz": mod_xyz.cpu().numpy(), "out:new_points": mod_points.cpu().numpy()}, 1e-3, name + " against the module")
    worst_ref = compare_case(got, ref, 1e-3, name + " against the recorded reference")
    assert np.array_equal(got["out:new_xyz"].view(np.uint32), ref["out:new_xyz"].view(np.uint32))
    print("%s: worst relative error %.3e against the module, %.3e against the reference" % (name, worst_mod[0], worst_ref[0]))
    # the default start is the module's
    a, b = fused(xyz, points), mod(xyz, points)
    assert torch.equal(a[0], b[0].detach())
    compare_case({"out:new_points": a[1].cpu().numpy()}, {"out:new_points": b[1].detach().cpu().numpy()}, 1e-3, name + ", default start")
    # new running statistics: stale until refresh()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.add_(0.25)
        moved = mod(xyz, points, start=start)[1]
    assert torch.equal(fused(xyz, points, start=start)[1].view(torch.int32), new_points.view(torch.int32))
    fresh = fused.refresh()(xyz, points, start=start)[1]
    compare_case({"out:new_points": fresh.cpu().numpy()}, {"out:new_points": moved.cpu().numpy()}, 1e-3, name + ", refreshed")
    assert not torch.equal(fresh, new_points)


def test_wrapper_refuses_train_mode_and_falls_back_outside_the_envelope(hip_device):
    from svnet_amd import sa_fused as SF
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    dev = hip_device
    mod, xyz, points, start, _ = _golden_module("single", dev)
    fused = SF.FusedSetAbstraction(mod)
    mod.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(xyz, points, start=start)
    mod.eval()
    with pytest.raises(ValueError, match="xyz requires grad"):
        fused(xyz.clone().requires_grad_(), points, start=start)
    # a layer of 300 channels is outside the kernel's limits: the module's own forward, bit for bit
    torch.manual_seed(5)
    wide = PointNetSetAbstraction(8, 0.4, 8, 3, [16, 300], False).to(dev).eval()
    fused = SF.FusedSetAbstraction(wide)
    x = FL.dev(dev, G.gauss_case(12, B, 64, 4, 0)[0].transpose(0, 2, 1))[0]
    assert not fused.supported(64, 0) and SF.FusedSetAbstraction(mod).supported(256, 4)
    got, want = fused(x, None), wide(x, None)
    assert tuple(got[1].shape) == (B, 300, 8) and not got[1].requires_grad
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].detach().view(torch.int32))


def test_wrapper_in_a_captured_graph(hip_device):
    """The multi-scale wrapper with a device start captured on a side stream after a warm-up; two replays with the inputs refilled
    in place between them each give the eager result bit for bit."""
    from svnet_amd import sa_fused as SF
    from svnet_amd.models.utils.pointnet_msg import PointNetSetAbstractionMsg
    dev = hip_device
    N, S, D = 300, 33, 5
    torch.manual_seed(9)
    mod = PointNetSetAbstractionMsg(S, [0.4, 0.1, 0.4], [16, 4, 70], D, [[12, 20], [8], [16, 16, 7]]).to(dev).eval()
    fused = SF.FusedSetAbstraction(mod)
    sets = []
    for seed in (90, 91):
        x, _, pts = G.gauss_case(seed, B, N, 4, D)
        sets.append(FL.dev(dev, x.transpose(0, 2, 1), pts.transpose(0, 2, 1), np.array([seed % 7, 200 + seed % 5], dtype=np.int64)))
    x, pts, start = (t.clone() for t in sets[0])

    def run():
        return fused(x, pts, start=start)

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
        for dst, src in zip((x, pts, start), s):
            dst.copy_(src)
        res[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = [r.clone() for r in res]
        eager = run()
        for a, b in zip(replayed, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.isnan(a).any()
        compare_case({"out:new_points": replayed[1].cpu().numpy()}, {"out:new_points": mod(x, pts, start=start)[1].detach().cpu().numpy()}, 1e-3,
                     "captured against the module")
