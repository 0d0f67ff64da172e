"""GPU tests (-m gpu) of the part-segmentation vector-neuron path: svnet_vn_edge2_mean_f32 (svnet_amd/csrc/vn_edge2.hip) through
svnet_amd.vn_fused.vn_edge2_mean, svnet_vn_std_coords_f32 (csrc/vn_tail.hip) through svnet_amd.vn_tail.vn_std_coords, and the wrapper
svnet_amd.vn_pseg.FusedVNDGCNNPSeg - against the numpy restatement tests/vn_pseg_ref.py, the modules' own eval forward and the
reference's recorded run (tests/golden/vn_pseg.npz).  The contracts are fixed sequences of single-rounded operations, so the kernels'
results are compared as BIT PATTERNS (a -0 counted as +0); whatever goes through the modules, which round differently, within the
project's activation tolerance tests.common.compare_case(..., 1e-3).  Every reference is computed once per process and shared."""
import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_pseg_cases as PC
from tests import vn_pseg_ref as P
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import compare_case

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = PC.GOLDEN
_once = FL.cache()

# (C, O1, O2, N, k, B, share1, share2, slope): the model's first level; its second; k = 1 with K padded and N no multiple of 16;
# k = 15 / 16 / 17 (one tile short, full, two tiles) with k = N and three clouds; every width 1 and N = 1; k = 40 (three tiles) with a
# shared direction in layer 1; k = 64 (four tiles), the widest O2, a shared direction in layer 2, slope 0; the widest O1 with both
# directions shared and eight clouds (the XCD order); and the largest image of a point, 128 channels x four tiles: more than 64 KB of LDS.
CASES = [(1, 21, 21, 64, 8, 2, False, False, 0.2),
         (21, 21, 21, 64, 8, 2, False, False, 0.2),
         (2, 3, 5, 17, 1, 2, False, False, 0.2),
         (4, 6, 7, 15, 15, 2, False, False, 0.2),
         (4, 6, 7, 16, 16, 2, False, False, 0.2),
         (4, 6, 7, 33, 17, 3, False, False, 0.2),
         (5, 1, 1, 1, 1, 2, False, False, 0.2),
         (21, 42, 22, 40, 40, 2, True, False, 0.2),
         (8, 70, 128, 70, 64, 1, False, True, 0.0),
         (3, 128, 5, 20, 4, 8, True, True, 0.2),
         (4, 128, 4, 64, 64, 1, False, False, 0.2)]


def _arrays(C, O1, O2, N, k, B, share1, share2, lists="random"):
    """(x [B,C,3,N], idx [B,N,k], layer 1's arrays, layer 2's): weights ~ N(0, 1/K), BatchNorm weights of both signs, statistics away
    from identity.  lists "repeated": every edge of a point goes to one neighbour; "outside": entries from -N to 2N."""
    def make():
        seed = 8600 + 97 * C + 7 * O1 + O2
        x = synth.normal(seed, 1, (B, C, 3, N))
        idx = synth.integers(seed, 2, (B, N, k), N)
        if lists == "repeated":
            idx = np.ascontiguousarray(np.broadcast_to(idx[:, :, :1], idx.shape))
        elif lists == "outside":
            idx = synth.integers(seed, 9, (B, N, k), 3 * N) - N
            assert (idx < 0).any() and (idx >= N).any()
        return x, idx, VC.layer_arrays(seed, 2 * C, O1, 1 if share1 else O1, signs=4), VC.layer_arrays(seed + 1, O1, O2, 1 if share2 else O2, signs=5)
    return _once(("arrays", C, O1, O2, N, k, B, share1, share2, lists), make)


def _folds(a1, a2):
    keys = ("w_feat", "w_dir", "gamma", "beta", "mean", "var")
    return V.fold(*(a1[key] for key in keys)), T.fold_point(*(a2[key] for key in keys))


def _want(C, O1, O2, N, k, B, share1, share2, slope, lists="random"):
    def make():
        x, idx, a1, a2 = _arrays(C, O1, O2, N, k, B, share1, share2, lists)
        f1, f2 = _folds(a1, a2)
        return P.level2_batch(x, idx, f1, f2, slope, slope)
    return _once(("want", C, O1, O2, N, k, B, share1, share2, slope, lists), make)


def _folded(dev, C, O1, O2, share1, share2, slope, a1, a2):
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    return VF.fold_vn_layer(VC.layer(dev, 2 * C, O1, share1, slope, a1)), VT.fold_vn_point(VC.layer(dev, O1, O2, share2, slope, a2))


@pytest.mark.parametrize("C,O1,O2,N,k,B,share1,share2,slope", CASES, ids=lambda v: str(v))
def test_two_layer_level_equals_the_restatement_bit_for_bit(C, O1, O2, N, k, B, share1, share2, slope, hip_device):
    from svnet_amd import vn_fused as VF
    dev = hip_device
    x, idx, a1, a2 = _arrays(C, O1, O2, N, k, B, share1, share2)
    want = _want(C, O1, O2, N, k, B, share1, share2, slope)
    f1, f2 = _folded(dev, C, O1, O2, share1, share2, slope, a1, a2)
    assert VF.supported2(N, k, C, O1, f1.Od, O2, f2.Od) and (f1.Od, f2.Od) == (1 if share1 else O1, 1 if share2 else O2)
    tx, tidx = FL.dev(dev, x, idx)
    tag = "C %d O1 %d O2 %d N %d k %d B %d share %s %s slope %s" % (C, O1, O2, N, k, B, share1, share2, slope)
    got = VF.vn_edge2_mean(tx, tidx, f1, f2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, O2, 3, N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    buf = torch.full((B, O2, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VF.vn_edge2_mean(tx, tidx, f1, f2, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    # one cloud on its own (B 1) has the bits it has inside the batch; the workspace kept from the larger call is reused, and a
    # second full call on it gives the first one's bits
    ws = f1.workspace
    FL.same_bits(VF.vn_edge2_mean(tx[B - 1:].contiguous(), tidx[B - 1:].contiguous(), f1, f2), want[B - 1:], tag + ", one cloud alone")
    FL.same_bits(VF.vn_edge2_mean(tx, tidx, f1, f2), want, tag + ", second call")
    assert f1.workspace is ws
    # the float64 form of the modules' definition, and the modules themselves, within the project's tolerance
    f64 = np.stack([P.level2_f64(x[b], idx[b], a1, a2, slope, slope) for b in range(B)])
    compare_case({"out": got.cpu().numpy()}, {"out": f64}, 1e-3, tag + ", against float64")
    from svnet_amd.models.utils.vn_util import get_graph_feature
    with torch.no_grad():
        mod = f2.layer(f1.layer(get_graph_feature(tx, k=k, idx=tidx))).mean(dim=-1)
    compare_case({"out": got.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the modules")


@pytest.mark.parametrize("lists", ["repeated", "outside"])
def test_lists_with_repeated_and_out_of_range_entries(lists, hip_device):
    """Out-of-range entries (-N .. 2N) are clamped into the cloud, as the restatement clamps them; a repeated neighbour is summed k times."""
    from svnet_amd import vn_fused as VF
    C, O1, O2, N, k, B, slope = 4, 9, 6, 23, 6, 2, 0.2
    x, idx, a1, a2 = _arrays(C, O1, O2, N, k, B, False, False, lists)
    want = _want(C, O1, O2, N, k, B, False, False, slope, lists)
    f1, f2 = _folded(hip_device, C, O1, O2, False, False, slope, a1, a2)
    tx, tidx = FL.dev(hip_device, x, idx)
    FL.same_bits(VF.vn_edge2_mean(tx, tidx, f1, f2), want, lists)
    if lists == "outside":
        FL.same_bits(VF.vn_edge2_mean(tx, tidx.clamp(0, N - 1), f1, f2), want, "clamped by the caller")


# (C, Cy, N, B): the model's widths at one run; every size 1; a run plus one point, three clouds; the widest C
COORD_CASES = [(63, 170, 64, 2), (1, 1, 1, 1), (5, 3, 65, 3), (512, 4, 16, 2)]


@pytest.mark.parametrize("C,Cy,N,B", COORD_CASES, ids=lambda v: str(v))
def test_std_coords_equal_the_restatement_and_the_pooled_entry_bit_for_bit(C, Cy, N, B, hip_device):
    from svnet_amd import vn_tail as VT
    dev = hip_device

    def make():
        seed = 9700 + 11 * C + Cy + N
        x, y = synth.normal(seed, 1, (B, C, 3, N)), synth.normal(seed, 3, (B, Cy, 3, N))
        w_lin = (synth.normal(seed, 4, (3, Cy)) / np.sqrt(F32(Cy))).astype(F32)
        return x, y, w_lin, np.stack([P.std_coords(x[b], y[b], w_lin) for b in range(B)])
    x, y, w_lin, want = _once(("coords", C, Cy, N, B), make)
    assert VT.supported_coords(N, C, Cy)
    tx, ty, tw = FL.dev(dev, x, y, w_lin)
    tag = "C %d Cy %d N %d B %d" % (C, Cy, N, B)
    got = VT.vn_std_coords(tx, ty, tw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 3 * C, N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    buf = torch.full((B, 3 * C, N), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_std_coords(tx, ty, tw, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    FL.same_bits(VT.vn_std_coords(tx[B - 1:].contiguous(), ty[B - 1:].contiguous(), tw), want[B - 1:], tag + ", one cloud alone")
    # the pooled entry states the same two rules: its amax half is the maximum over n of these coordinates
    h = VT.vn_std_pool(tx, ty, tw)
    FL.same_bits(got.amax(dim=-1), h[:, :3 * C].cpu().numpy(), tag + ", amax against vn_std_pool")
    f64 = np.stack([P.std_coords_f64(x[b], y[b], w_lin) for b in range(B)])
    compare_case({"out": got.cpu().numpy()}, {"out": f64}, 1e-3, tag + ", against float64")


# ---- the model
def _inputs(dev):
    x, l = FL.dev(dev, GOLDEN["x"], GOLDEN["l"])
    return x, l, [FL.dev(dev, i)[0] for i in PC.lists()]


def test_wrapper_equals_the_module_and_the_recorded_run(hip_device, monkeypatch):
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_pseg as VP
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.utils import vn_util as U
    dev = hip_device
    seed, B, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    fused = VP.FusedVNDGCNNPSeg(model)
    assert fused.fused and fused.supported(B, N, k) and not fused.supported(B, N, 65) and not fused.supported(B, 32769, k) and not fused.training
    x, l, lists = _inputs(dev)
    got = fused(x, l, idx=lists)
    assert tuple(got.shape) == (B, num_part, N) and not got.requires_grad and all(a is b for a, b in zip(fused.last_idx, lists))
    with torch.no_grad():
        mod = model(x, l, idx=lists)
    w_ref = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "against the module")
    print("worst relative error %.3e against the reference, %.3e against the module" % (w_ref[0], w_mod[0]))
    # the two-layer levels against the restatement, bit for bit, and the recorded levels, on the recorded inputs
    st = PC.state()
    h = GOLDEN["x"][:, None]
    for i in (0, 1):
        f1, f2 = V.fold_state(st, P.LEVEL_PREFIXES[i][0]), T.fold_point_state(st, P.LEVEL_PREFIXES[i][1])
        want = _once(("golden level", i), lambda: P.level2_batch(h, GOLDEN["idx%d" % i], f1, f2))
        out = VF.vn_edge2_mean(FL.dev(dev, h)[0], lists[i], *fused.levels[i])
        FL.same_bits(out, want, "level %d" % i)
        compare_case({"out": out.cpu().numpy()}, {"out": GOLDEN["lvl%d" % i]}, 1e-3, "level %d against the recorded one" % i)
        h = want
    # the coordinates on the recorded levels: against the restatement bit for bit, against the recorded ones within the tolerance
    x123, y = PC.frame_inputs()
    want = _once("golden coords", lambda: np.stack([P.std_coords(x123[b], y[b], st["std_feature.vn_lin.weight"]) for b in range(B)]))
    e = VT.vn_std_coords(*FL.dev(dev, x123, y), model.std_feature.vn_lin.weight.detach())
    FL.same_bits(e, want, "coordinates")
    compare_case({"out": e.cpu().numpy()}, {"out": GOLDEN["coords"]}, 1e-3, "coordinates against the recorded ones")
    # the dynamic graphs: last_idx equals the lists the model's own forward builds, and replayed into it gives the same logits
    got = fused(x, l)
    assert len(fused.last_idx) == 3 and all(tuple(i.shape) == (B, N, k) and i.dtype == torch.int64 for i in fused.last_idx)
    own, knn = [], U.knn
    monkeypatch.setattr(U, "knn", lambda feat, k: own.append(knn(feat, k)) or own[-1])
    with torch.no_grad():
        dyn = model(x, l)
    monkeypatch.undo()
    assert len(own) == 3 and all(torch.equal(a, b) for a, b in zip(fused.last_idx, own))
    assert torch.equal(own[0].cpu(), torch.from_numpy(GOLDEN["idx0"]))
    compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": dyn.cpu().numpy()}, 1e-3, "dynamic graphs, against the module")
    # two runs are bit-identical
    again = fused(x, l)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # new running statistics and a new conv8: stale until refresh()
    with torch.no_grad():
        model.conv4.batchnorm.bn.running_mean.add_(0.25)
        model.conv8[0].weight.mul_(0.5)
        moved = model(x, l, idx=lists)
    fresh = fused.refresh()(x, l, idx=lists)
    compare_case({"out:logits": fresh.cpu().numpy()}, {"out:logits": moved.cpu().numpy()}, 1e-3, "refreshed")
    assert fused.release() is fused


def test_wrapper_in_a_captured_graph(hip_device):
    """The whole fused forward, k-NN included, captured on a side stream after a warm-up; replays with the inputs refilled in place
    between them each give the eager result bit for bit."""
    from svnet_amd import vn_pseg as VP
    dev = hip_device
    seed, B, N, k, num_part = P.GOLDEN_CASE
    fused = VP.FusedVNDGCNNPSeg(PC.golden_model(dev))
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
    from svnet_amd import vn_pseg as VP
    dev = hip_device
    seed, B, N, k, num_part = P.GOLDEN_CASE
    x, l, lists = _inputs(dev)
    torch.manual_seed(11)
    pooled = PC.golden_model(dev, "max")
    fused = VP.FusedVNDGCNNPSeg(pooled)
    assert not fused.fused and not fused.levels and not fused.supported(B, N, k) and fused.refresh() is fused
    with torch.no_grad():
        want = pooled(x, l, idx=lists)
    assert torch.equal(fused(x, l, idx=lists).view(torch.int32), want.view(torch.int32))
    # a level outside the limits: lists of 65 neighbours (k <= 64) through a mean-pooled model
    model = PC.golden_model(dev)
    fused = VP.FusedVNDGCNNPSeg(model)
    wide = [FL.dev(dev, synth.integers(12, i, (B, N, 65), N))[0] for i in range(3)]
    with torch.no_grad():
        want = model(x, l, idx=wide)
    got = fused(x, l, idx=wide)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got.requires_grad
    # normalize_frame: the Gram-Schmidt frame is not what the kernels compute
    framed = PC.golden_model(dev)
    framed.std_feature.normalize_frame = True
    fused_framed = VP.FusedVNDGCNNPSeg(framed)
    assert not fused_framed.fused
    with torch.no_grad():
        want = framed(x, l, idx=lists)
    assert torch.equal(fused_framed(x, l, idx=lists).view(torch.int32), want.view(torch.int32))
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(x, l, idx=lists)
    model.eval()
    with pytest.raises(ValueError, match="x requires grad"):
        fused(x.clone().requires_grad_(), l, idx=lists)
    with pytest.raises(ValueError, match=r"l must be \[B,16\]"):
        fused(x, l[:, :8].contiguous(), idx=lists)
    with pytest.raises(ValueError, match="three levels"):
        fused(x, l, idx=lists[:2])


def test_distiller_takes_the_fused_teacher_for_a_segmentation_step(hip_device):
    """Distiller(FusedVNDGCNNPSeg(model), (x, l), seg=True) runs forward-only on the student's input buffers and its logits feed
    kd_seg_loss."""
    from svnet_amd import vn_pseg as VP
    from svnet_amd.train import Distiller, kd_seg_loss
    dev = hip_device
    seed, B, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model(dev)
    x, l, _ = _inputs(dev)
    d = Distiller(VP.FusedVNDGCNNPSeg(model), (x, l), seg=True)
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
