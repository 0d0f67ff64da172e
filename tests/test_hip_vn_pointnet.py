"""GPU tests (-m gpu) of the vector-neuron PointNet path: svnet_vn_cross_fold_f32 and svnet_vn_edge_cross_mean_f32
(svnet_amd/csrc/vn_cross.hip) through svnet_amd.vn_pointnet, the norm-only point layer svnet_vn_point_norm_f32
(svnet_amd/csrc/vn_tail.hip) through svnet_amd.vn_tail, and the wrapper FusedVNPointNet, against the numpy restatement
tests/vn_pointnet_ref.py, the modules' own eval forward and the reference's recorded run (tests/golden/vn_pointnet.npz).  The contracts
are fixed sequences of single-rounded operations, so the kernels' results are compared as BIT PATTERNS (a -0 counted as +0); whatever
goes through the modules, which round differently, within the project's activation tolerance tests.common.compare_case(..., 1e-3).
Every reference is computed once per process and shared.  Nothing here provokes a fault: every index the kernels form is clamped or
masked, and the tests check values only."""
import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_pointnet_cases as PC
from tests import vn_pointnet_ref as P
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import compare_case

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = PC.GOLDEN


def _cross_folded(dev, O, share, slope, a, f):
    """The FoldedVNCross on the device; the fold's results are checked as bit patterns on the way."""
    from svnet_amd import vn_pointnet as VP
    folded = VP.fold_vn_cross(VC.layer(dev, 3, O, share, slope, a))
    Od = 1 if share else O
    got = folded.folded.cpu().numpy()
    W = np.concatenate([f["Wf"], f["Wd"]], axis=0)
    assert (folded.O, folded.Od) == (O, Od) and got.shape == (3 * (O + Od) + 2 * O,) and folded.slope == slope
    assert np.array_equal(got[:W.size].view(np.uint32), W.ravel().view(np.uint32)), "W"
    assert np.array_equal(got[W.size:W.size + O].view(np.uint32), f["s"].view(np.uint32)), "s"
    assert np.array_equal(got[W.size + O:].view(np.uint32), f["t"].view(np.uint32)), "t"
    return folded


@pytest.mark.parametrize("B,N,k,O,share,slope,lists", PC.CROSS_CASES, ids=lambda v: str(v))
def test_cross_level_equals_the_restatement_bit_for_bit(B, N, k, O, share, slope, lists, hip_device):
    from svnet_amd import vn_pointnet as VP
    dev = hip_device
    x, idx, a = PC.cross_arrays(B, N, k, O, share, lists)
    f, want = PC.cross_want(B, N, k, O, share, slope, lists)
    folded = _cross_folded(dev, O, share, slope, a, f)
    tx, tidx = FL.dev(dev, x, idx)
    tag = "B %d N %d k %d O %d share %s slope %s %s" % (B, N, k, O, share, slope, lists)
    got = VP.vn_edge_cross_mean(tx, tidx, folded)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, O, 3, N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    buf = torch.full((B, O, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VP.vn_edge_cross_mean(tx, tidx, folded, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    if lists == "outside":
        assert (idx == -1).any() and (idx == N + 5).any()
        FL.same_bits(VP.vn_edge_cross_mean(tx, tidx.clamp(0, N - 1), folded), want, "clamped by the caller")
    # one cloud on its own (B 1) has the bits it has inside the batch
    FL.same_bits(VP.vn_edge_cross_mean(tx[B - 1:].contiguous(), tidx[B - 1:].contiguous(), folded), want[B - 1:], tag + ", one cloud alone")
    # against the module's own eval forward on the edge feature, within the project's tolerance
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross
    with torch.no_grad():
        mod = folded.layer(get_graph_feature_cross(tx, k=k, idx=tidx.clamp(0, N - 1))).mean(dim=-1)
    compare_case({"out": got.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the module")


def test_cross_level_at_the_origin_and_on_duplicated_points(hip_device):
    from svnet_amd import vn_pointnet as VP
    x, idx = P.degenerate_cloud()
    a = VC.layer_arrays(5, 3, 21, 21)
    f = P.fold_cross(*(a[key] for key in PC.KEYS))
    want = P.cross_level_batch(x[:, None], idx, f, 0.0)
    assert np.isfinite(want).all()
    tx, tidx = FL.dev(hip_device, x[:, None], idx)
    FL.same_bits(VP.vn_edge_cross_mean(tx, tidx, _cross_folded(hip_device, 21, False, 0.0, a, f)), want, "origin and duplicates")


def test_cross_level_refuses_what_it_cannot_take_and_follows_refresh(hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_pointnet as VP
    B, N, k, O, share, slope = 2, 33, 5, 7, False, 0.2
    x, idx, a = PC.cross_arrays(B, N, k, O, share)
    f, want = PC.cross_want(B, N, k, O, share, slope)
    folded = _cross_folded(hip_device, O, share, slope, a, f)
    tx, tidx = FL.dev(hip_device, x, idx)
    with torch.no_grad():
        folded.layer.batchnorm.bn.running_mean.add_(0.25)
    FL.same_bits(VP.vn_edge_cross_mean(tx, tidx, folded), want, "stale until refresh()")
    moved = dict(a, mean=(a["mean"] + F32(0.25)).astype(F32))
    FL.same_bits(VP.vn_edge_cross_mean(tx, tidx, folded.refresh()), P.cross_level_batch(x, idx, P.fold_cross(*(moved[key] for key in PC.KEYS)), slope), "refreshed")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VP.vn_edge_cross_mean(tx.cpu(), tidx.cpu(), folded)
    with pytest.raises(_lib.SvnetHipError, match="not supported"):                # k > N
        VP.vn_edge_cross_mean(tx[:, :, :, :4].contiguous(), tidx[:, :4].contiguous(), folded)


@pytest.mark.parametrize("N", PC.NORM_POINTS)
@pytest.mark.parametrize("C,O", PC.NORM_WIDTHS, ids=lambda v: str(v))
def test_norm_only_point_layer_equals_the_restatement_bit_for_bit(C, O, N, hip_device):
    from svnet_amd import vn_tail as VT
    dev, B = hip_device, 2
    x, a = PC.norm_arrays(C, O, N)
    f, want = PC.norm_want(C, O, N)
    linear, norm = PC.norm_layers(dev, C, O, a)
    folded = VT.fold_vn_linear_norm(linear, norm)
    got = folded.folded.cpu().numpy()
    assert (folded.C, folded.O) == (C, O) and got.shape == (C * O + 2 * O,)
    assert np.array_equal(got[:C * O].view(np.uint32), np.ascontiguousarray(f["Wf"].T).ravel().view(np.uint32)), "WT"
    assert np.array_equal(got[C * O:C * O + O].view(np.uint32), f["s"].view(np.uint32)) and np.array_equal(got[C * O + O:].view(np.uint32), f["t"].view(np.uint32))
    tx = FL.dev(dev, x)[0]
    tag = "C %d O %d N %d" % (C, O, N)
    out = VT.vn_point_norm(tx, folded)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, O, 3, N) and out.is_contiguous()
    FL.same_bits(out, want, tag)
    buf = torch.full((B, O, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_point_norm(tx, folded, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    with torch.no_grad():
        mod = norm(linear(tx))
    compare_case({"out": out.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the modules")
    if (C, O) == PC.NORM_WIDTHS[0]:
        # the leaky form with slope 1.0 is the identity behind the norm wherever its dot >= 0: both run the same chain and norm
        p, d = T._chain(x[0], f["Wf"]), T._chain(x[0], a["w_dir"])
        dot = V.norm_leaky(p, d, f["s"], f["t"], 1.0)[1]                          # [N,O]
        leaky = VT.vn_point(tx, VT.fold_vn_point(VC.layer(dev, C, O, False, 1.0, a, dim=4)))
        keep = np.broadcast_to((dot >= 0).T[:, None, :], want[0].shape)
        assert np.array_equal(FL.bits(leaky[0])[keep], FL.bits(want[0])[keep]), tag + ", vn_point with slope 1.0"
    # new statistics: stale until refresh()
    with torch.no_grad():
        norm.bn.running_var.mul_(2.0)
    FL.same_bits(VT.vn_point_norm(tx, folded), want, tag + ", stale until refresh()")
    moved = P.fold_norm(a["w_feat"], a["gamma"], a["beta"], a["mean"], (a["var"] * F32(2)).astype(F32))
    FL.same_bits(VT.vn_point_norm(tx, folded.refresh()), np.stack([P.point_norm(x[b], moved) for b in range(B)]), tag + ", refreshed")


# ---- the model
def _inputs(dev):
    return FL.dev(dev, GOLDEN["x"], GOLDEN["idx"])


def test_fused_model_equals_the_module_and_the_recorded_logits(hip_device):
    from svnet_amd import vn_pointnet as VP
    dev = hip_device
    seed, B, N, k, num_class = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    fused = VP.FusedVNPointNet(model)
    assert fused.fused and fused.supported(B, N, k) and not fused.supported(B, N, 65) and not fused.supported(B, 4, k) and not fused.training
    x, idx = _inputs(dev)
    got = fused(x, idx=idx)
    assert tuple(got.shape) == (B, num_class) and not got.requires_grad and fused.last_idx is idx
    with torch.no_grad():
        mod = model(x, idx=idx)
    w_ref = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "against the module")
    print("worst relative error %.3e against the reference, %.3e against the module" % (w_ref[0], w_mod[0]))
    # the stages: in front of the transform net's torch layers bit for bit the restatement, behind them within the tolerance
    h, st = fused.encode(x, idx)
    want = PC.restated()
    FL.same_bits(st["pos"], want["pos"], "the position level")
    FL.same_bits(st["conv1"], want["conv1"], "conv1")
    stages = {"out:" + key: st[key].cpu().numpy() for key in ("pos", "conv1", "fstn", "conv2")}
    stages["out:h"] = h.cpu().numpy()
    compare_case(stages, {key: GOLDEN[key[4:]] for key in stages}, 1e-3, "the stages against the recorded ones")
    compare_case({"out": st["local"].cpu().numpy()}, {"out": want["local"]}, 1e-3, "conv3 + bn3 against the restatement")
    # the dynamic graph: last_idx is the recorded list, and replayed into the module gives the same logits
    dyn = fused(x)
    assert tuple(fused.last_idx.shape) == (B, N, k) and fused.last_idx.dtype == torch.int64
    assert torch.equal(fused.last_idx.cpu(), torch.from_numpy(GOLDEN["idx"]))
    with torch.no_grad():
        mod = model(x, idx=fused.last_idx)
    compare_case({"out:logits": dyn.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "dynamic graph, against the module")
    # two eager calls return the same bits
    assert torch.equal(dyn.view(torch.int32), fused(x).view(torch.int32)) and torch.equal(dyn.view(torch.int32), got.view(torch.int32))
    # new running statistics in a layer of each kind: stale until refresh()
    with torch.no_grad():
        model.feat.conv_pos.batchnorm.bn.running_mean.add_(0.25)
        model.feat.bn3.bn.running_var.mul_(1.5)
        model.feat.fstn.conv2.batchnorm.bn.running_mean.add_(0.25)
        moved = model(x, idx=idx)
    assert torch.equal(fused(x, idx=idx).view(torch.int32), got.view(torch.int32))
    fresh = fused.refresh()(x, idx=idx)
    compare_case({"out:logits": fresh.cpu().numpy()}, {"out:logits": moved.cpu().numpy()}, 1e-3, "refreshed")
    assert float((fresh - got).abs().max()) > 0 and fused.release() is fused


def test_wrapper_in_a_captured_graph(hip_device):
    """The whole fused forward, k-NN included, captured on a side stream after a warm-up; replays with the input refilled in place
    between them each give the eager result bit for bit."""
    from svnet_amd import vn_pointnet as VP
    dev = hip_device
    seed, B, N, k, num_class = P.GOLDEN_CASE
    fused = VP.FusedVNPointNet(PC.golden_model(dev))
    gx, _ = _inputs(dev)
    other = FL.dev(dev, synth.cloud_batch(96, 0, 0, B, N))[0]
    x = gx.clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        fused(x)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = fused(x)
    for src in (other, gx):
        x.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = fused(x)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and not torch.isnan(out).any()
    compare_case({"out:logits": out.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "the last replay against the recorded logits")


def test_fallbacks_equal_the_module_bit_for_bit_and_train_mode_is_refused(hip_device):
    from svnet_amd import vn_pointnet as VP
    dev = hip_device
    seed, B, N, k, num_class = P.GOLDEN_CASE
    x, idx = _inputs(dev)
    torch.manual_seed(11)
    pooled = PC.golden_model(dev, "max")
    fused = VP.FusedVNPointNet(pooled)
    assert not fused.fused and not fused.supported(B, N, k) and fused.refresh() is fused
    with torch.no_grad():
        want = pooled(x, idx=idx)
    assert torch.equal(fused(x, idx=idx).view(torch.int32), want.view(torch.int32))
    # outside the limits: a list of 65 neighbours (k <= 64) through a mean-pooled model
    model = PC.golden_model(dev)
    fused = VP.FusedVNPointNet(model)
    wide = FL.dev(dev, synth.integers(12, 0, (B, N, 65), N))[0]
    with torch.no_grad():
        want = model(x, idx=wide)
    got = fused(x, idx=wide)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got.requires_grad
    # normalize_frame: the Gram-Schmidt frame is not what the kernels compute
    framed = PC.golden_model(dev)
    framed.feat.std_feature.normalize_frame = True
    fused_framed = VP.FusedVNPointNet(framed)
    assert not fused_framed.fused
    with torch.no_grad():
        want = framed(x, idx=idx)
    assert torch.equal(fused_framed(x, idx=idx).view(torch.int32), want.view(torch.int32))
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(x, idx=idx)
    model.eval()
    with pytest.raises(ValueError, match="x requires grad"):
        fused(x.clone().requires_grad_(), idx=idx)
    with pytest.raises(ValueError, match="neighbour list"):
        fused(x, idx=idx[:, :8].contiguous())


def test_distiller_takes_the_fused_teacher(hip_device):
    """Distiller(FusedVNPointNet(model), (x,)) runs forward-only on the student's input buffer and its logits feed kd_loss."""
    from svnet_amd import vn_pointnet as VP
    from svnet_amd.train import Distiller, kd_loss
    dev = hip_device
    seed, B, N, k, num_class = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    x, _ = _inputs(dev)
    d = Distiller(VP.FusedVNPointNet(model), (x,))
    logits = d.run()
    assert tuple(logits.shape) == (B, num_class) and not logits.requires_grad and not any(p.requires_grad for p in model.parameters())
    with torch.no_grad():
        mod = model(x, idx=d.model.last_idx)
    compare_case({"out:logits": logits.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "the teacher's logits")
    student = torch.from_numpy(synth.normal(5, 1, (B, num_class))).to(dev).requires_grad_()
    target = torch.from_numpy(synth.class_labels(5, 0, 0, B, num_class)).to(dev)
    loss = d.loss_fn(student, target)
    want = kd_loss(student.detach(), logits, target)
    assert torch.isfinite(loss) and abs(float(loss.detach()) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    loss.backward()
    assert student.grad is not None and bool(torch.isfinite(student.grad).all())
