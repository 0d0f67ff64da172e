"""GPU tests (-m gpu) of the fused vector-neuron tail: the svnet_vn_point_*, svnet_vn_cloud_mean_f32 and svnet_vn_std_pool_* entries
(svnet_amd/csrc/vn_tail.hip) through svnet_amd.vn_tail, against the numpy restatement tests/vn_tail_ref.py, the modules' own eval
forward and the reference's recorded run (tests/golden/vn.npz).  The contract is a fixed sequence of single-rounded operations, so the
kernels' results are compared as BIT PATTERNS (a -0 counted as +0); whatever goes through the modules, which round differently, within
the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every reference is computed once per process and shared."""
import argparse

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fused_level_cases as FL
from tests import vn_cases as VC
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import compare_case

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN, _state, _golden_model, _levels = VC.GOLDEN, VC.state, VC.golden_model, VC.levels
_once = FL.cache()

# (C, Cg, O, Od, N, B): the smallest case; K and N off the tile multiples; more than 64 columns with one direction row and a cloud
# term; B % 8 == 0; the model's widths (conv5's, and vn1's with its cloud term); and a K at which a workgroup takes 32 points with O
# direction rows and whole float4s along n - the one form of the kernel the other cases do not reach.
POINT_CASES = [(1, 0, 1, 1, 1, 1), (5, 0, 7, 7, 9, 2), (3, 2, 70, 1, 130, 3), (6, 5, 20, 20, 33, 8), (169, 0, 341, 1, 64, 2), (341, 341, 341, 341, 33, 2),
               (120, 3, 20, 20, 40, 2)]
# (C, Cg, Cy, N): a single run, an exact run, a run plus one, three runs with a short last one; the model's widths at one run
STD_CASES = [(C, Cg, Cy, N) for C, Cg, Cy in ((5, 5, 3), (4, 0, 6)) for N in (1, 64, 65, 130)] + [(341, 341, 170, 64)]
STD_B = 2


def _point_arrays(C, Cg, O, Od, N, B):
    """(x [B,C,3,N], g [B,Cg,3], the layer's arrays): weights ~ N(0, 1/K), BatchNorm weights of both signs, statistics away from identity."""
    def make():
        seed = 9100 + 13 * C + 7 * Cg + O
        return synth.normal(seed, 1, (B, C, 3, N)), synth.normal(seed, 2, (B, Cg, 3)), VC.layer_arrays(seed, C + Cg, O, Od, signs=7)
    return _once(("point arrays", C, Cg, O, Od, N, B), make)


def _point_want(C, Cg, O, Od, N, B, slope):
    def make():
        x, g, a = _point_arrays(C, Cg, O, Od, N, B)
        f = T.fold_point(a["w_feat"], a["w_dir"], a["gamma"], a["beta"], a["mean"], a["var"])
        return f, np.stack([T.point_level(x[b], f, slope, g[b] if Cg else None) for b in range(B)])
    return _once(("point want", C, Cg, O, Od, N, B, slope), make)


def _folded(dev, C, Cg, O, Od, slope, a, f):
    """The FoldedVNPoint on the device; the fold's results are checked as bit patterns on the way."""
    from svnet_amd import vn_tail as VT
    folded = VT.fold_vn_point(VC.layer(dev, C + Cg, O, Od == 1 and O != 1, slope, a, dim=4), Cg)
    K, R = C + Cg, O + Od
    got = folded.folded.cpu().numpy()
    WT = np.ascontiguousarray(np.concatenate([f["Wf"], f["Wd"]], axis=0).T)          # [K][W_f | W_d]
    assert (folded.C, folded.Cg, folded.O, folded.Od) == (C, Cg, O, Od) and got.shape == (K * R + 2 * O,)
    assert np.array_equal(got[:K * R].view(np.uint32), WT.ravel().view(np.uint32)), "WT"
    assert np.array_equal(got[K * R:K * R + O].view(np.uint32), f["s"].view(np.uint32)), "s"
    assert np.array_equal(got[K * R + O:].view(np.uint32), f["t"].view(np.uint32)), "t"
    return folded


@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("C,Cg,O,Od,N,B", POINT_CASES, ids=lambda v: str(v))
def test_point_level_equals_the_restatement_bit_for_bit(C, Cg, O, Od, N, B, slope, hip_device):
    from svnet_amd import vn_tail as VT
    dev = hip_device
    x, g, a = _point_arrays(C, Cg, O, Od, N, B)
    f, want = _point_want(C, Cg, O, Od, N, B, slope)
    folded = _folded(dev, C, Cg, O, Od, slope, a, f)
    tx, tg = FL.dev(dev, x, g if Cg else None)
    tag = "C %d Cg %d O %d Od %d N %d B %d slope %s" % (C, Cg, O, Od, N, B, slope)
    got = VT.vn_point(tx, folded, cloud=tg)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, O, 3, N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    buf = torch.full((B, O, 3, N), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_point(tx, folded, cloud=tg, out=buf) is buf
    FL.same_bits(buf, want, tag + ", into out")
    # one cloud on its own (B 1) has the bits it has inside the batch; the workspace kept from the larger call is reused
    ws = folded.workspace
    alone = VT.vn_point(tx[B - 1:].contiguous(), folded, cloud=None if tg is None else tg[B - 1:].contiguous())
    FL.same_bits(alone, want[B - 1:], tag + ", one cloud alone")
    assert folded.workspace is ws
    # against the module's own eval forward on the explicitly expanded input, within the project's tolerance
    with torch.no_grad():
        full = tx if tg is None else torch.cat((tx, tg.unsqueeze(-1).expand(B, Cg, 3, N)), dim=1)
        mod = folded.layer(full)
    compare_case({"out": got.cpu().numpy()}, {"out": mod.cpu().numpy()}, 1e-3, tag + ", against the module")


def _std_arrays(C, Cg, Cy, N):
    def make():
        seed = 9500 + 11 * C + 5 * Cg + Cy + N
        x, g = synth.normal(seed, 1, (STD_B, C, 3, N)), synth.normal(seed, 2, (STD_B, Cg, 3))
        y, w_lin = synth.normal(seed, 3, (STD_B, Cy, 3, N)), (synth.normal(seed, 4, (3, Cy)) / np.sqrt(F32(Cy))).astype(F32)
        want = np.stack([T.std_pool(x[b], y[b], w_lin, g[b] if Cg else None) for b in range(STD_B)])
        return x, g, y, w_lin, want, T.ordered_mean(x)
    return _once(("std", C, Cg, Cy, N), make)


@pytest.mark.parametrize("C,Cg,Cy,N", STD_CASES, ids=lambda v: str(v))
def test_cloud_mean_and_std_pool_equal_the_restatement_bit_for_bit(C, Cg, Cy, N, hip_device):
    from svnet_amd import _lib
    from svnet_amd import vn_tail as VT
    dev = hip_device
    x, g, y, w_lin, want, want_mean = _std_arrays(C, Cg, Cy, N)
    tx, tg, ty, tw = FL.dev(dev, x, g if Cg else None, y, w_lin)
    tag = "C %d Cg %d Cy %d N %d" % (C, Cg, Cy, N)
    m = VT.vn_cloud_mean(tx)
    assert tuple(m.shape) == (STD_B, C, 3) and m.dtype == torch.float32
    FL.same_bits(m, want_mean, tag + ", cloud mean")
    buf = torch.full((STD_B, C, 3), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_cloud_mean(tx, out=buf) is buf
    FL.same_bits(buf, want_mean, tag + ", cloud mean into out")
    compare_case({"out": m.cpu().numpy()}, {"out": x.astype(np.float64).mean(-1)}, 1e-3, tag + ", cloud mean against float64")
    # the workspace pre-filled with NaN: every partial the finish reads was written by this call
    ws = VT._Workspace(dev)
    ws.take(int(_lib.lib().svnet_vn_std_pool_workspace_bytes(STD_B, N, C, Cg))).fill_(255)
    out = torch.full((STD_B, 6 * (C + Cg)), float("nan"), dtype=torch.float32, device=dev)
    assert VT.vn_std_pool(tx, ty, tw, cloud=tg, out=out, workspace=ws) is out
    FL.same_bits(out, want, tag + ", std-pool")
    FL.same_bits(VT.vn_std_pool(tx, ty, tw, cloud=tg), want, tag + ", std-pool, shared workspace")
    FL.same_bits(VT.vn_std_pool(tx[1:].contiguous(), ty[1:].contiguous(), tw, cloud=None if tg is None else tg[1:].contiguous()), want[1:],
                 tag + ", one cloud alone")
    f64 = np.stack([T.std_pool_f64(T.expanded(x[b], g[b]) if Cg else x[b], y[b], w_lin) for b in range(STD_B)])
    compare_case({"out": out.cpu().numpy()}, {"out": f64}, 1e-3, tag + ", std-pool against float64")


# ---- the model
def _golden_pooled():
    return _once("golden pooled", lambda: T.pooled(_levels(), _state()))


def test_tail_on_the_recorded_levels_equals_the_restatement_the_module_and_the_recorded_logits(hip_device):
    from svnet_amd import vn_tail as VT
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    model = _golden_model(dev)
    tail = VT.FusedVNTail(model)
    assert tail.fused and tail.supported(B, N) and not tail.supported(B, 32769) and not tail.training
    assert tuple(tail.widths) == T.MODEL_POINT and (tail.widths[0][2], tail.widths[0][2], tail.Cy) == T.MODEL_STD
    feats = list(FL.dev(dev, *_levels()))
    h = tail.pooled(feats)
    assert tuple(h.shape) == (B, 6 * 682)
    FL.same_bits(h, _golden_pooled(), "the tail in front of the head")
    got = tail(feats)
    assert tuple(got.shape) == (B, num_class) and not got.requires_grad
    with torch.no_grad():
        mod = model.tail(feats)
    w_ref = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "against model.tail")
    print("worst relative error %.3e against the reference, %.3e against model.tail" % (w_ref[0], w_mod[0]))


def test_fused_model_with_the_fused_tail_equals_the_one_without_and_the_recorded_logits(hip_device):
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    dev = hip_device
    model = _golden_model(dev)
    fused, plain = VF.FusedVNDGCNN(model, tail=True), VF.FusedVNDGCNN(model)
    assert isinstance(fused.tail, VT.FusedVNTail) and plain.tail is None and list(fused.state_dict()) == list(plain.state_dict())
    x = FL.dev(dev, GOLDEN["x"])[0]
    lists = [FL.dev(dev, GOLDEN["idx%d" % i])[0] for i in range(4)]
    got, base = fused(x, idx=lists), plain(x, idx=lists)
    compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": base.cpu().numpy()}, 1e-3, "against tail=False")
    compare_case({"out:logits": got.cpu().numpy()}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    compare_case({"out:logits": fused(x).cpu().numpy()}, {"out:logits": plain(x).cpu().numpy()}, 1e-3, "dynamic graphs")
    assert fused.release() is fused


def test_refresh_follows_changed_parameters(hip_device):
    from svnet_amd import vn_fused as VF
    dev = hip_device
    model = _golden_model(dev)
    fused = VF.FusedVNDGCNN(model, tail=True)
    feats = list(FL.dev(dev, *_levels()))
    with torch.no_grad():
        model.conv5.batchnorm.bn.running_mean.add_(0.25)
        model.std_feature.vn2.map_to_feat.weight.mul_(0.5)
    FL.same_bits(fused.tail.pooled(feats), _golden_pooled(), "stale until refresh()")
    moved = dict(_state())
    moved["conv5.batchnorm.bn.running_mean"] = (moved["conv5.batchnorm.bn.running_mean"] + F32(0.25)).astype(F32)
    moved["std_feature.vn2.map_to_feat.weight"] = (moved["std_feature.vn2.map_to_feat.weight"] * F32(0.5)).astype(F32)
    assert fused.refresh() is fused                                               # (through the wrapper: it reaches the tail)
    FL.same_bits(fused.tail.pooled(feats), T.pooled(_levels(), moved), "refreshed")


def test_tail_in_a_captured_graph(hip_device):
    """The tail captured on a side stream after a warm-up; two replays with the inputs refilled in place between them each give the
    eager result bit for bit."""
    from svnet_amd import vn_tail as VT
    dev = hip_device
    tail = VT.FusedVNTail(_golden_model(dev))
    sets = [list(FL.dev(dev, *_levels())), [torch.from_numpy(synth.normal(95, i, l.shape)).to(dev) for i, l in enumerate(_levels())]]
    feats = [t.clone() for t in sets[0]]
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        tail.pooled(feats)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = tail.pooled(feats)
    for s in (sets[1], sets[0]):
        for dst, src in zip(feats, s):
            dst.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = tail.pooled(feats)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and not torch.isnan(out).any()
    FL.same_bits(out, _golden_pooled(), "the last replay")


def test_fallbacks_equal_the_module_bit_for_bit_and_train_mode_is_refused(hip_device, monkeypatch):
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    from svnet_amd.models import vn_dgcnn_cls
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    feats = list(FL.dev(dev, *_levels()))
    # normalize_frame: the Gram-Schmidt frame is not what the kernel computes
    model = _golden_model(dev)
    model.std_feature.normalize_frame = True
    tail = VT.FusedVNTail(model)
    assert not tail.fused and not tail.layers and not tail.supported(B, N)
    with torch.no_grad():
        want = model.tail(feats)
    got = tail(feats)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got.requires_grad
    with pytest.raises(VT._lib.SvnetHipError, match="outside the fused tail"):
        tail.pooled(feats)
    # a width above the limits: a model whose global width is 520 > 512
    monkeypatch.setattr(vn_dgcnn_cls, "GLOBAL_WIDTH", 520)
    torch.manual_seed(12)
    wide = vn_dgcnn_cls.VN_DGCNN_CLS(argparse.Namespace(k=k, pooling="mean"), num_class).to(dev).eval()
    monkeypatch.undo()
    tail = VT.FusedVNTail(wide)
    assert not tail.fused
    small = [f[:, :, :, :8].contiguous() for f in feats]
    with torch.no_grad():
        want = wide.tail(small)
    assert torch.equal(tail(small).view(torch.int32), want.view(torch.int32))
    # pooling = 'max' with tail=True: nothing is folded, every call is the model's
    torch.manual_seed(11)
    pooled = _golden_model(dev, "max")
    fused = VF.FusedVNDGCNN(pooled, tail=True)
    assert fused.tail is None and not fused.levels
    x = FL.dev(dev, GOLDEN["x"])[0]
    lists = [FL.dev(dev, GOLDEN["idx%d" % i])[0] for i in range(4)]
    with torch.no_grad():
        want = pooled(x, idx=lists)
    assert torch.equal(fused(x, idx=lists).view(torch.int32), want.view(torch.int32))
    # train mode
    model = _golden_model(dev)
    tail = VT.FusedVNTail(model)
    fused = VF.FusedVNDGCNN(model, tail=True)
    model.train()
    with pytest.raises(RuntimeError, match="train mode"):
        tail(feats)
    with pytest.raises(RuntimeError, match="train mode"):
        fused(x, idx=lists)
    model.eval()
    with pytest.raises(ValueError, match=r"feats\[1\] requires grad"):
        tail([f.clone().requires_grad_() if i == 1 else f for i, f in enumerate(feats)])


def test_distiller_takes_the_fused_teacher_with_the_fused_tail(hip_device):
    from svnet_amd import vn_fused as VF
    from svnet_amd.train import Distiller
    dev = hip_device
    seed, B, N, k, num_class = V.GOLDEN_CASE
    model = _golden_model(dev)
    x = FL.dev(dev, GOLDEN["x"])[0]
    d = Distiller(VF.FusedVNDGCNN(model, tail=True), (x,))
    logits = d.run()
    assert tuple(logits.shape) == (B, num_class) and not logits.requires_grad
    with torch.no_grad():
        mod = model(x, idx=d.model.last_idx)
    compare_case({"out:logits": logits.cpu().numpy()}, {"out:logits": mod.cpu().numpy()}, 1e-3, "the teacher's logits")
