"""GPU tests (-m gpu) of the vector tail's wide envelope - the svnet_vn_*_wide_* entries of svnet_amd/csrc/vn_tail.hip through
svnet_amd.vn_tail with wide=True - and of the wrapper svnet_amd.vn_pointnet_pseg.FusedVNPointNetPSeg, against the numpy restatements
(tests/vn_tail_ref.py, tests/vn_pointnet_ref.py, tests/vn_pseg_ref.py, chained in tests/vn_pointnet_pseg_ref.py), the entries of the
base envelope, the module's own eval forward and the reference's recorded run (tests/golden/vn_pointnet_pseg.npz).  The contracts are
fixed sequences of single-rounded operations, so the kernels' results are compared as BIT PATTERNS (a -0 counted as +0); whatever goes
through the modules, which round differently, within the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every
reference is computed once per process and shared.  Nothing here provokes a fault: every shape lies inside the envelope it is sent
to, and the tests check values only."""
import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_pointnet_cases as CLS
from tests import vn_pointnet_pseg_cases as PC
from tests import vn_pointnet_pseg_ref as P
from tests.common import compare_case

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = PC.GOLDEN
B = PC.B


def _folded(dev, C, Cg, O, Od, slope, a, f=None, wide=True):
    """The FoldedVNPoint on the device, folded in the envelope asked for; with f the fold's results are checked as bit patterns."""
    from svnet_amd import vn_tail as VT
    folded = VT.fold_vn_point(VC.layer(dev, C + Cg, O, Od == 1 and O != 1, slope, a, dim=4), Cg, wide=wide)
    assert (folded.C, folded.Cg, folded.O, folded.Od, folded.wide) == (C, Cg, O, Od, wide)
    if f is not None:
        K, R = C + Cg, O + Od
        got = folded.folded.cpu().numpy()
        WT = np.ascontiguousarray(np.concatenate([f["Wf"], f["Wd"]], axis=0).T)
        assert got.shape == (K * R + 2 * O,) and np.array_equal(got[:K * R].view(np.uint32), WT.ravel().view(np.uint32)), "WT"
        assert np.array_equal(got[K * R:K * R + O].view(np.uint32), f["s"].view(np.uint32)) and np.array_equal(got[K * R + O:].view(np.uint32), f["t"].view(np.uint32))
    return folded


@pytest.mark.parametrize("N", PC.WIDE_POINT_N)
@pytest.mark.parametrize("C,Cg,O,Od,slope", PC.WIDE_POINT, ids=lambda v: str(v))
def test_wide_point_level_equals_the_restatement_bit_for_bit(C, Cg, O, Od, slope, N, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    dev = hip_device
    x, g, a = PC.point_arrays(C, Cg, O, Od, N)
    f, want = PC.point_want(C, Cg, O, Od, N, slope)
    folded = _folded(dev, C, Cg, O, Od, slope, a, f)
    tx, tg = FL.dev(dev, x, g if Cg else None)
    tag = "wide: C %d Cg %d O %d Od %d N %d slope %s" % (C, Cg, O, Od, N, slope)
    buf = torch.full((B, O, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_point(tx, folded, cloud=tg, out=buf) is buf
    FL.same_bits(buf, want, tag)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    # one cloud on its own has the bits it has inside the batch
    FL.same_bits(VT.vn_point(tx[1:].contiguous(), folded, cloud=None if tg is None else tg[1:].contiguous()), want[1:], tag + ", one cloud alone")
    if N == PC.WIDE_POINT_N[0]:
        # the same layer unasked is refused as before, and the message names the base envelope
        with pytest.raises(_lib.SvnetHipError, match=r"C <= 512, Cg <= 512, 1 <= O <= 512"):
            _folded(dev, C, Cg, O, Od, slope, a, wide=False)


def test_wide_point_level_on_both_staging_paths(hip_device):
    """N % 4 == 0: x is staged in float4s when it is 16-byte aligned, float by float when it is not; both give the restatement's bits."""
    from svnet_amd import vn_tail as VT
    dev = hip_device
    C, Cg, O, Od, slope, N = PC.WIDE_VEC
    x, g, a = PC.point_arrays(C, Cg, O, Od, N)
    f, want = PC.point_want(C, Cg, O, Od, N, slope)
    folded = _folded(dev, C, Cg, O, Od, slope, a, f)
    tx = FL.dev(dev, x)[0]
    assert N % 4 == 0 and tx.data_ptr() % 16 == 0
    FL.same_bits(VT.vn_point(tx, folded), want, "float4 staging")
    flat = torch.empty(tx.numel() + 1, dtype=torch.float32, device=dev)
    view = flat[1:].view(tx.shape)
    view.copy_(tx)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    FL.same_bits(VT.vn_point(view, folded), want, "a view that is not 16-byte aligned")


@pytest.mark.parametrize("N", PC.WIDE_NORM_N)
@pytest.mark.parametrize("C,O", PC.WIDE_NORM, ids=lambda v: str(v))
def test_wide_norm_only_layer_equals_the_restatement_bit_for_bit(C, O, N, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    dev = hip_device
    x, a = PC.norm_arrays(C, O, N)
    f, want = PC.norm_want(C, O, N)
    linear, norm = CLS.norm_layers(dev, C, O, a)
    folded = VT.fold_vn_linear_norm(linear, norm, wide=True)
    got = folded.folded.cpu().numpy()
    assert (folded.C, folded.O, folded.wide) == (C, O, True) and got.shape == (C * O + 2 * O,)
    assert np.array_equal(got[:C * O].view(np.uint32), np.ascontiguousarray(f["Wf"].T).ravel().view(np.uint32)), "WT"
    tx = FL.dev(dev, x)[0]
    tag = "wide norm only: C %d O %d N %d" % (C, O, N)
    out = VT.vn_point_norm(tx, folded)
    assert tuple(out.shape) == (B, O, 3, N) and out.is_contiguous()
    FL.same_bits(out, want, tag)
    with torch.no_grad():
        mod = norm(linear(tx))
    compare_case({"out": out.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the modules")
    with pytest.raises(_lib.SvnetHipError, match=r"1 <= C <= 512, 1 <= O <= 512"):
        VT.fold_vn_linear_norm(linear, norm)


@pytest.mark.parametrize("N", PC.RUN_N)
def test_wide_cloud_mean_equals_the_restatement_bit_for_bit(N, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    C = PC.WIDE_MEAN_C
    x, _, _, _, _, want = PC.std_arrays(C, 0, 4, N, want=False)
    tx = FL.dev(hip_device, x)[0]
    m = VT.vn_cloud_mean(tx, wide=True)
    assert tuple(m.shape) == (B, C, 3)
    FL.same_bits(m, want, "wide cloud mean, N %d" % N)
    compare_case({"out": m.cpu().numpy()}, {"out": x.astype(np.float64).mean(-1)}, 1e-3, "against float64")
    with pytest.raises(_lib.SvnetHipError, match=r"1 <= C <= 512"):
        VT.vn_cloud_mean(tx)


@pytest.mark.parametrize("N", PC.RUN_N)
@pytest.mark.parametrize("C,Cg,Cy", PC.WIDE_STD, ids=lambda v: str(v))
def test_wide_std_pool_equals_the_restatement_bit_for_bit(C, Cg, Cy, N, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    dev = hip_device
    x, g, y, w_lin, want, _ = PC.std_arrays(C, Cg, Cy, N)
    tx, tg, ty, tw = FL.dev(dev, x, g if Cg else None, y, w_lin)
    tag = "wide std-pool: C %d Cg %d Cy %d N %d" % (C, Cg, Cy, N)
    # the workspace pre-filled with NaN: every partial the finish reads was written by this call
    ws = VT._Workspace(dev)
    need = int(_lib.lib().svnet_vn_std_pool_wide_workspace_bytes(B, N, C, Cg))
    assert need == 2 * ((N + 63) // 64) * B * 3 * (C + Cg) * 4
    ws.take(need).fill_(255)
    out = torch.full((B, 6 * (C + Cg)), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_std_pool(tx, ty, tw, cloud=tg, out=out, workspace=ws, wide=True) is out and ws.buffer.numel() == need
    FL.same_bits(out, want, tag)
    FL.same_bits(VT.vn_std_pool(tx[1:].contiguous(), ty[1:].contiguous(), tw, cloud=None if tg is None else tg[1:].contiguous(), wide=True), want[1:],
                 tag + ", one cloud alone")
    if N == PC.RUN_N[0]:
        with pytest.raises(_lib.SvnetHipError, match=r"C, Cg, Cy <= 512"):
            VT.vn_std_pool(tx, ty, tw, cloud=tg)


@pytest.mark.parametrize("C,Cy", PC.WIDE_COORDS, ids=lambda v: str(v))
def test_wide_std_coords_equals_the_restatement_and_the_pool_bit_for_bit(C, Cy, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    dev, N = hip_device, 65
    x, _, y, w_lin, _, _ = PC.std_arrays(C, 0, Cy, N, want=False)
    want = PC.coords_want(C, Cy, N)
    tx, ty, tw = FL.dev(dev, x, y, w_lin)
    tag = "wide coordinates: C %d Cy %d N %d" % (C, Cy, N)
    out = torch.full((B, 3 * C, N), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_std_coords(tx, ty, tw, out=out, wide=True) is out
    FL.same_bits(out, want, tag)
    h = VT.vn_std_pool(tx, ty, tw, wide=True)
    FL.same_bits(out.amax(dim=-1), h[:, :3 * C].cpu().numpy(), tag + ", amax against the wide vn_std_pool")
    with pytest.raises(_lib.SvnetHipError, match=r"1 <= C, Cy <= 512"):
        VT.vn_std_coords(tx, ty, tw)


def _same(a, b, tag):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), tag
    assert not torch.isnan(a).any(), tag


@pytest.mark.parametrize("C,Cg,O,Od,N", PC.BOTH, ids=lambda v: str(v))
def test_wide_entries_equal_the_base_entries_bit_for_bit_inside_the_base_envelope(C, Cg, O, Od, N, hip_device):
    """Point, norm only, mean, pool and coordinates at shapes both envelopes admit: the twin runs its entry's kernel.  (The shape
    (341, 341, 682, 682) cannot be asked of a base entry - O = 682 is outside its envelope - so the first case carries the widest O the
    base envelope has, 512, over vn1's 341 + 341 input channels.)"""
    from svnet_amd import vn_tail as VT
    dev = hip_device
    slope = 0.2
    x, g, a = PC.point_arrays(C, Cg, O, Od, N)
    tx, tg = FL.dev(dev, x, g)
    tag = "C %d Cg %d O %d Od %d N %d" % (C, Cg, O, Od, N)
    base, wide = (_folded(dev, C, Cg, O, Od, slope, a, wide=w) for w in (False, True))
    _same(base.folded, wide.folded, tag + ", the fold")
    _same(VT.vn_point(tx, base, cloud=tg), VT.vn_point(tx, wide, cloud=tg), tag + ", point")
    xn, an = PC.norm_arrays(C, O, N)
    linear, norm = CLS.norm_layers(dev, C, O, an)
    txn = FL.dev(dev, xn)[0]
    _same(VT.vn_point_norm(txn, VT.fold_vn_linear_norm(linear, norm)), VT.vn_point_norm(txn, VT.fold_vn_linear_norm(linear, norm, wide=True)), tag + ", norm only")
    _same(VT.vn_cloud_mean(tx), VT.vn_cloud_mean(tx, wide=True), tag + ", mean")
    Cy = O
    ty = torch.from_numpy(synth.normal(31, 1, (B, Cy, 3, N))).to(dev)
    tw = torch.from_numpy((synth.normal(31, 2, (3, Cy)) / np.sqrt(F32(Cy))).astype(F32)).to(dev)
    _same(VT.vn_std_pool(tx, ty, tw, cloud=tg), VT.vn_std_pool(tx, ty, tw, cloud=tg, wide=True), tag + ", pool")
    _same(VT.vn_std_coords(tx, ty, tw), VT.vn_std_coords(tx, ty, tw, wide=True), tag + ", coordinates")


# ---- the model
def _inputs(dev):
    return FL.dev(dev, GOLDEN["x"], GOLDEN["l"], GOLDEN["idx"])


def test_wrapper_equals_the_restatement_the_module_and_the_recorded_run(hip_device):
    from svnet_amd import vn_pointnet_pseg as VP
    dev = hip_device
    seed, _, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    fused = VP.FusedVNPointNetPSeg(model)
    assert fused.fused and fused.supported(B, N, k) and not fused.supported(B, N, 65) and not fused.supported(B, 4, k) and not fused.supported(B, 32769, k)
    assert not fused.training and fused.norm.wide and fused.points["vn1"].wide and fused.points["vn2"].wide and not fused.points["conv4"].wide
    x, l, idx = _inputs(dev)
    got = fused(x, l, idx=idx)
    assert tuple(got.shape) == (B, num_part, N) and not got.requires_grad and fused.last_idx is idx
    with torch.no_grad():
        mod = model(x, l, idx=idx)
    w_ref = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "against the module")
    print("worst relative error %.3e against the reference, %.3e against the module" % (w_ref[0], w_mod[0]))
    assert torch.equal(fused(x, l.unsqueeze(1), idx=idx).view(torch.int32), got.view(torch.int32))                # l as [B,1,16]
    # the stages: in front of the transform net's torch layers bit for bit the restatement; behind them bit for bit on the
    # restatement's own inputs, and within the tolerance as the wrapper chains them
    st = fused.encode(x, idx)
    want = PC.restated()
    for key in ("pos", "out1", "out2", "out3"):
        FL.same_bits(st[key], want[key], key)
    stages = {"out:" + key: P.recorded(key, st[key].cpu().numpy()) for key in ("pos", "out1", "out2", "out3", "out4", "fstn", "h")}
    e = st["e1234z"].cpu().numpy()
    stages["out:e1234"] = P.recorded("e1234", e[:, :P.SKIP])
    stages["out:trans"] = np.ascontiguousarray(e[:, P.SKIP:].reshape(B, 3, 3, N))                                # row 3 a + k
    compare_case(stages, {key: GOLDEN[key[4:]] for key in stages}, 1e-3, "the stages against the recorded ones")
    compare_case({"out": st["e5"].cpu().numpy()}, {"out": want["e5"]}, 1e-3, "the local coordinates against the restatement")
    _stages_behind_the_transform_net(fused, want, dev)
    # the dynamic graph: last_idx is the recorded list, and replayed into the module gives the same logits
    dyn = fused(x, l)
    assert tuple(fused.last_idx.shape) == (B, N, k) and fused.last_idx.dtype == torch.int64
    assert torch.equal(fused.last_idx.cpu(), torch.from_numpy(GOLDEN["idx"]))
    with torch.no_grad():
        mod = model(x, l, idx=fused.last_idx)
    compare_case({"out:logits": dyn.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "dynamic graph, against the module")
    assert torch.equal(dyn.view(torch.int32), fused(x, l).view(torch.int32)) and torch.equal(dyn.view(torch.int32), got.view(torch.int32))
    assert fused.release() is fused


def _stages_behind_the_transform_net(fused, want, dev):
    """The wrapper's own folded layers on the restatement's inputs: conv4 with the restated transform vectors, the wide conv5 + bn5,
    the wide std tail and both coordinate calls - each bit for bit the restatement's next stage."""
    from svnet_amd import vn_tail as VT
    Pt = fused.points
    out3, g, out4, local, y = FL.dev(dev, want["out3"], want["fstn"], want["out4"], want["local"], want["y"])
    w_lin = fused.model.std_feature.vn_lin.weight.detach()
    FL.same_bits(VT.vn_point(out3, Pt["conv4"], cloud=g), want["out4"], "conv4 with cloud = g")
    FL.same_bits(VT.vn_point_norm(out4, fused.norm), want["local"], "conv5 + bn5, wide")
    m, ty, h = VT.std_tail(local, Pt["vn1"], Pt["vn2"], w_lin, fused._std_ws, wide=True)
    FL.same_bits(m, want["m"], "the cloud mean, wide")
    FL.same_bits(ty, want["y"], "vn1 and vn2, wide")
    FL.same_bits(h[:, :P.POOLED], want["h"], "the amax half of the wide pool")
    skip = torch.cat(FL.dev(dev, want["out1"], want["out2"]) + (out3, out4, fused._units(PC.B, out3.shape[3], dev)), dim=1)
    e = VT.vn_std_coords(skip, y, w_lin)
    FL.same_bits(e[:, :P.SKIP], want["e1234"], "e1234")
    FL.same_bits(e[:, P.SKIP:].reshape(PC.B, 3, 3, -1), want["trans"], "the frame through the unit vectors")
    FL.same_bits(VT.vn_std_coords(local, y, w_lin, wide=True), want["e5"], "e5, wide")


def test_refresh_follows_a_changed_weight_and_a_changed_running_statistic(hip_device):
    from svnet_amd import vn_pointnet_pseg as VP
    dev = hip_device
    model = PC.golden_model(dev)
    fused = VP.FusedVNPointNetPSeg(model)
    x, l, idx = _inputs(dev)
    got = fused(x, l, idx=idx)
    with torch.no_grad():
        model.bn5.bn.running_var.mul_(1.5)                                        # the wide norm-only fold
        model.std_feature.vn1.batchnorm.bn.running_mean.add_(0.25)                # a wide point fold
        model.convs1.weight[:, 7000:].mul_(0.5)                                   # the mean block of the split head weight
        moved = model(x, l, idx=idx)
    assert torch.equal(fused(x, l, idx=idx).view(torch.int32), got.view(torch.int32)), "stale until refresh()"
    fresh = fused.refresh()(x, l, idx=idx)
    compare_case({"out:logits": fresh.cpu().numpy()}, {"out:logits": moved.cpu().numpy()}, 1e-3, "refreshed")
    assert float((fresh - got).abs().max()) > 0


def test_wrapper_in_a_captured_graph(hip_device):
    """The whole fused forward, k-NN included, captured on a side stream after a warm-up; two replays with the inputs refilled in place
    between them each give the eager result bit for bit."""
    from svnet_amd import vn_pointnet_pseg as VP
    dev = hip_device
    seed, _, N, k, num_part = P.GOLDEN_CASE
    fused = VP.FusedVNPointNetPSeg(PC.golden_model(dev))
    gx, gl, _ = _inputs(dev)
    other = FL.dev(dev, synth.cloud_batch(96, 0, 0, B, N), synth.category_onehot(96, 0, 0, B))
    x, l = gx.clone(), gl.clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        fused(x, l)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = fused(x, l)
    for sx, sl in (other, (gx, gl)):
        x.copy_(sx)
        l.copy_(sl)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = fused(x, l)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and not torch.isnan(out).any()
    compare_case({"out:logits": out.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "the last replay against the recorded logits")


def test_fallbacks_equal_the_module_bit_for_bit_and_train_mode_is_refused(hip_device):
    from svnet_amd import vn_pointnet_pseg as VP
    dev = hip_device
    seed, _, N, k, num_part = P.GOLDEN_CASE
    x, l, idx = _inputs(dev)
    torch.manual_seed(11)
    pooled = PC.golden_model(dev, "max")
    fused = VP.FusedVNPointNetPSeg(pooled)
    assert not fused.fused and not fused.supported(B, N, k) and fused.refresh() is fused
    with torch.no_grad():
        want = pooled(x, l, idx=idx)
    assert torch.equal(fused(x, l, idx=idx).view(torch.int32), want.view(torch.int32))
    # outside the limits: a list of 65 neighbours (k <= 64) through a mean-pooled model
    model = PC.golden_model(dev)
    fused = VP.FusedVNPointNetPSeg(model)
    wide = FL.dev(dev, synth.integers(12, 0, (B, N, 65), N))[0]
    with torch.no_grad():
        want = model(x, l, idx=wide)
    got = fused(x, l, idx=wide)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got.requires_grad
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(x, l, idx=idx)
    model.eval()
    with pytest.raises(ValueError, match="x requires grad"):
        fused(x.clone().requires_grad_(), l, idx=idx)
    with pytest.raises(ValueError, match=r"l must be \[B,16\]"):
        fused(x, l[:, :8].contiguous(), idx=idx)
    with pytest.raises(ValueError, match="neighbour list"):
        fused(x, l, idx=idx[:, :8].contiguous())


def test_distiller_takes_the_fused_teacher_for_a_segmentation_step(hip_device):
    """Distiller(FusedVNPointNetPSeg(model), (x, l), seg=True) runs forward-only on the student's input buffers and its logits feed
    kd_seg_loss."""
    from svnet_amd import vn_pointnet_pseg as VP
    from svnet_amd.train import Distiller, kd_seg_loss
    dev = hip_device
    seed, _, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    x, l, _ = _inputs(dev)
    d = Distiller(VP.FusedVNPointNetPSeg(model), (x, l), seg=True)
    logits = d.run()
    assert tuple(logits.shape) == (B, num_part, N) and not logits.requires_grad and not any(p.requires_grad for p in model.parameters())
    with torch.no_grad():
        mod = model(x, l, idx=d.model.last_idx)
    compare_case({"out:logits": logits.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "the teacher's logits")
    student = torch.from_numpy(synth.normal(5, 1, (B, num_part, N))).to(dev).requires_grad_()
    target = torch.from_numpy(synth.integers(5, 2, (B, N), num_part)).to(dev)
    loss = d.loss_fn(student, target)
    want = kd_seg_loss(student.detach(), logits, target)
    assert torch.isfinite(loss) and abs(float(loss.detach()) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    loss.backward()
    assert student.grad is not None and bool(torch.isfinite(student.grad).all())
