"""GPU tests (-m gpu) of the fused vector-neuron edge level: svnet_vn_fold_f32, svnet_vn_tables_f32 and svnet_vn_edge_mean_f32
(svnet_amd/csrc/vn_edge.hip) through svnet_amd.vn_fused, against the numpy restatement tests/vn_ref.py, the module's own eval forward
and the reference's recorded run (tests/golden/vn.npz).  The contract is a fixed sequence of single-rounded operations, so the
kernels' results are compared as BIT PATTERNS (a -0 counted as +0); the wrapper against the module, which rounds differently, within
the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every reference is computed once per process and shared."""
import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_ref as V
from tests.common import compare_case

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN, _state, _golden_model = VC.GOLDEN, VC.state, VC.golden_model
_once = FL.cache()

# (C, O, N, k, B, share, slope): the first level (K of one); the second; the widest level at an N that is no multiple of the 16 points
# of a workgroup or the 16 pairs of a table wave, three clouds (cloud boundaries, no XCD order); one neighbour; k = N; N = 1; one
# direction row; slope 0; eight clouds (the XCD order) of more than one workgroup each.
CASES = [(1, 21, 64, 8, 2, False, 0.2),
         (21, 21, 64, 8, 2, False, 0.2),
         (42, 85, 130, 20, 3, False, 0.2),
         (3, 1, 16, 1, 2, False, 0.2),
         (5, 7, 9, 9, 2, False, 0.2),
         (2, 5, 1, 1, 2, False, 0.2),
         (21, 42, 33, 8, 2, True, 0.2),
         (4, 6, 20, 5, 2, False, 0.0),
         (3, 70, 35, 4, 8, True, 0.0)]


def _arrays(C, O, N, k, B, share, lists="random"):
    """(x [B,C,3,N], idx [B,N,k], the layer's arrays): weights ~ N(0, 1/2C), BatchNorm weights of both signs, statistics away from
    identity.  lists "repeated": every edge of a point goes to one neighbour; "outside": entries from -N to 2N."""
    def make():
        seed = 8000 + 97 * C + O
        x = synth.normal(seed, 1, (B, C, 3, N))
        idx = synth.integers(seed, 2, (B, N, k), N)
        if lists == "repeated":
            idx = np.ascontiguousarray(np.broadcast_to(idx[:, :, :1], idx.shape))
        elif lists == "outside":
            idx = synth.integers(seed, 9, (B, N, k), 3 * N) - N
            assert (idx < 0).any() and (idx >= N).any()
        return x, idx, VC.layer_arrays(seed, 2 * C, O, 1 if share else O, signs=4)
    return _once(("arrays", C, O, N, k, B, share, lists), make)


def _want(C, O, N, k, B, share, slope, lists="random"):
    def make():
        x, idx, a = _arrays(C, O, N, k, B, share, lists)
        f = V.fold(a["w_feat"], a["w_dir"], a["gamma"], a["beta"], a["mean"], a["var"])
        return f, V.level_batch(x, idx, f, slope)
    return _once(("want", C, O, N, k, B, share, slope, lists), make)


def _folded(dev, C, O, share, slope, a, f):
    """The FoldedVNLayer on the device; the fold's results are checked as bit patterns on the way."""
    from svnet_amd import vn_fused as VF
    folded = VF.fold_vn_layer(VC.layer(dev, 2 * C, O, share, slope, a))
    Od, R = (1 if share else O), 2 * (O + (1 if share else O))
    got = folded.folded.cpu().numpy()
    WT = np.concatenate([f["Af"], f["Ad"], f["Df"], f["Dd"]], axis=0).T            # [C][A_f | A_d | D_f | D_d]
    assert (folded.C, folded.O, folded.Od) == (C, O, Od) and got.shape == (C * R + 2 * O,)
    assert np.array_equal(got[:C * R].view(np.uint32), np.ascontiguousarray(WT).ravel().view(np.uint32)), "WT"
    assert np.array_equal(got[C * R:C * R + O].view(np.uint32), f["s"].view(np.uint32)), "s"
    assert np.array_equal(got[C * R + O:].view(np.uint32), f["t"].view(np.uint32)), "t"
    return folded


@pytest.mark.parametrize("C,O,N,k,B,share,slope", CASES, ids=lambda v: str(v))
def test_level_equals_the_restatement_bit_for_bit(C, O, N, k, B, share, slope, hip_device):
    from svnet_amd import vn_fused as VF
    dev = hip_device
    x, idx, a = _arrays(C, O, N, k, B, share)
    f, want = _want(C, O, N, k, B, share, slope)
    folded = _folded(dev, C, O, share, slope, a, f)
    tx, tidx = FL.dev(dev, x, idx)
    tag = "C %d O %d N %d k %d B %d share %s slope %s" % (C, O, N, k, B, share, slope)
    got = VF.vn_edge_mean(tx, tidx, folded)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, O, 3, N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    buf = torch.full((B, O, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VF.vn_edge_mean(tx, tidx, folded, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    # one cloud on its own (B 1) has the bits it has inside the batch; the workspace kept from the larger call is reused
    ws = folded.workspace
    FL.same_bits(VF.vn_edge_mean(tx[B - 1:].contiguous(), tidx[B - 1:].contiguous(), folded), want[B - 1:], tag + ", one cloud alone")
    assert folded.workspace is ws
    # against the module's own eval forward on the edge feature, within the project's tolerance
    from svnet_amd.models.utils.vn_util import get_graph_feature
    with torch.no_grad():
        mod = folded.layer(get_graph_feature(tx, k=k, idx=tidx.clamp(0, N - 1))).mean(dim=-1)
    compare_case({"out": got.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the module")


@pytest.mark.parametrize("lists", ["repeated", "outside"])
def test_lists_with_repeated_and_out_of_range_entries(lists, hip_device):
    """Out-of-range entries are clamped into the cloud, as the restatement clamps them; a repeated neighbour is summed k times."""
    from svnet_amd import vn_fused as VF
    C, O, N, k, B, share, slope = 4, 9, 23, 6, 2, False, 0.2
    x, idx, a = _arrays(C, O, N, k, B, share, lists)
    f, want = _want(C, O, N, k, B, share, slope, lists)
    folded = _folded(hip_device, C, O, share, slope, a, f)
    tx, tidx = FL.dev(hip_device, x, idx)
    FL.same_bits(VF.vn_edge_mean(tx, tidx, folded), want, lists)
    if lists == "outside":
        FL.same_bits(VF.vn_edge_mean(tx, tidx.clamp(0, N - 1), folded), want, "clamped by the caller")


def test_refresh_follows_new_statistics_and_device_refusals(hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_fused as VF
    C, O, N, k, B, share, slope = 4, 6, 20, 5, 2, False, 0.0
    x, idx, a = _arrays(C, O, N, k, B, share)
    f, want = _want(C, O, N, k, B, share, slope)
    folded = _folded(hip_device, C, O, share, slope, a, f)
    tx, tidx = FL.dev(hip_device, x, idx)
    with torch.no_grad():
        folded.layer.batchnorm.bn.running_mean.add_(0.25)
    FL.same_bits(VF.vn_edge_mean(tx, tidx, folded), want, "stale until refresh()")
    moved = dict(a, mean=(a["mean"] + F32(0.25)).astype(F32))
    f2 = V.fold(moved["w_feat"], moved["w_dir"], moved["gamma"], moved["beta"], moved["mean"], moved["var"])
    FL.same_bits(VF.vn_edge_mean(tx, tidx, folded.refresh()), V.level_batch(x, idx, f2, slope), "refreshed")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.vn_edge_mean(tx.cpu(), tidx.cpu(), folded)
    with pytest.raises(_lib.SvnetHipError, match="not supported"):                # k > N
        VF.vn_edge_mean(tx[:, :, :, :4].contiguous(), tidx[:, :4].contiguous(), folded)


def test_level_in_a_captured_graph(hip_device):
    """The level captured on a side stream after a warm-up; two replays with the inputs refilled in place between them each give the
    eager result bit for bit."""
    from svnet_amd import vn_fused as VF
    dev = hip_device
    C, O, N, k, B, share, slope = 21, 42, 33, 8, 2, True, 0.2
    _, _, a = _arrays(C, O, N, k, B, share)
    f, _ = _want(C, O, N, k, B, share, slope)
    folded = _folded(dev, C, O, share, slope, a, f)
    sets = [FL.dev(dev, synth.normal(seed, 1, (B, C, 3, N)), synth.integers(seed, 2, (B, N, k), N)) for seed in (90, 91)]
    x, idx = (t.clone() for t in sets[0])
    out = torch.empty(B, O, 3, N, dtype=torch.float32, device=dev)

    def run(dst):
        return VF.vn_edge_mean(x, idx, folded, out=dst)

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run(out)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        run(out)
    for s in (sets[1], sets[0]):
        for dst, src in zip((x, idx), s):
            dst.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = run(torch.empty_like(out))
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and not torch.isnan(out).any()
        FL.same_bits(eager, V.level_batch(x.cpu().numpy(), idx.cpu().numpy(), f, slope), "eager")


# ---- the model
def test_knn_list_of_the_first_level_equals_the_recorded_one(hip_device):
    from svnet_amd.models.utils import vn_util as U
    seed, B, N, k, num_class = V.GOLDEN_CASE
    x = FL.dev(hip_device, GOLDEN["x"])[0]
    assert np.array_equal(U.knn(x, k).cpu().numpy(), GOLDEN["idx0"])


def test_fused_model_equals_the_module_and_the_recorded_logits(hip_device):
    from svnet_amd import vn_fused as VF
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    model = _golden_model(dev)
    fused = VF.FusedVNDGCNN(model)
    assert fused.supported(N, k) and not fused.supported(N, 65) and not fused.training
    x = FL.dev(dev, GOLDEN["x"])[0]
    # the recorded lists replayed: against the recorded logits and the module
    lists = [FL.dev(dev, GOLDEN["idx%d" % i])[0] for i in range(4)]
    got = fused(x, idx=lists)
    assert tuple(got.shape) == (B, num_class) and not got.requires_grad and all(a is b for a, b in zip(fused.last_idx, lists))
    with torch.no_grad():
        mod = model(x, idx=lists)
    w_ref = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "against the module")
    print("worst relative error %.3e against the reference, %.3e against the module" % (w_ref[0], w_mod[0]))
    # the levels themselves against the restatement, bit for bit, on the recorded inputs
    state = _state()
    h = GOLDEN["x"][:, None]
    for i, prefix in enumerate(V.LEVEL_PREFIXES):
        want = _once(("golden level", i), lambda: V.level_batch(h, GOLDEN["idx%d" % i], V.fold_state(state, prefix)))
        FL.same_bits(VF.vn_edge_mean(FL.dev(dev, h)[0], lists[i], fused.levels[i]), want, "level %d" % i)
        h = want
    # the dynamic graphs: last_idx replayed into the module
    got = fused(x)
    assert len(fused.last_idx) == 4 and all(tuple(i.shape) == (B, N, k) and i.dtype == torch.int64 for i in fused.last_idx)
    assert torch.equal(fused.last_idx[0].cpu(), torch.from_numpy(GOLDEN["idx0"]))
    with torch.no_grad():
        mod = model(x, idx=fused.last_idx)
    compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "dynamic graphs, against the module")
    # new running statistics: stale until refresh()
    with torch.no_grad():
        model.conv2.batchnorm.bn.running_mean.add_(0.25)
        moved = model(x, idx=lists)
    assert torch.equal(fused(x, idx=lists).view(torch.int32), fused(x, idx=lists).view(torch.int32))
    fresh = fused.refresh()(x, idx=lists)
    compare_case({"out:logits": fresh.cpu().numpy()}, {"out:logits": moved.cpu().numpy()}, 1e-3, "refreshed")


def test_fallbacks_equal_the_module_bit_for_bit_and_train_mode_is_refused(hip_device):
    from svnet_amd import vn_fused as VF
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    x = FL.dev(dev, GOLDEN["x"])[0]
    lists = [FL.dev(dev, GOLDEN["idx%d" % i])[0] for i in range(4)]
    torch.manual_seed(11)
    pooled = _golden_model(dev, "max")
    fused = VF.FusedVNDGCNN(pooled)
    assert not fused.levels and not fused.supported(N, k)
    with torch.no_grad():
        want = pooled(x, idx=lists)
    assert torch.equal(fused(x, idx=lists).view(torch.int32), want.view(torch.int32))
    # a level outside the limits: lists of 65 neighbours (k <= 64) through a mean-pooled model
    model = _golden_model(dev)
    fused = VF.FusedVNDGCNN(model)
    wide = [FL.dev(dev, synth.integers(12, i, (B, N, 65), N))[0] for i in range(4)]
    assert not fused.supported(N, 65)
    with torch.no_grad():
        want = model(x, idx=wide)
    got = fused(x, idx=wide)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got.requires_grad
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(x, idx=lists)
    model.eval()
    with pytest.raises(ValueError, match="x requires grad"):
        fused(x.clone().requires_grad_(), idx=lists)


def test_distiller_takes_the_fused_teacher(hip_device):
    """Distiller(FusedVNDGCNN(model), (x,)) runs forward-only on the student's input buffer and its logits feed kd_loss."""
    from svnet_amd import vn_fused as VF
    from svnet_amd.train import Distiller, kd_loss
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    model = _golden_model(dev)
    x = FL.dev(dev, GOLDEN["x"])[0]
    d = Distiller(VF.FusedVNDGCNN(model), (x,))
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
