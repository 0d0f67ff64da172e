"""CPU tests of the part-segmentation vector-neuron path: the torch model svnet_amd.models.VN_DGCNN_PSEG against the reference's
recorded run (tests/golden/vn_pseg.npz), the numpy restatement tests/vn_pseg_ref.py against the same recordings and the float64 direct
forms, the header's new entry points, and the refusals of vn_fused.vn_edge2_mean, vn_tail.vn_std_coords and vn_pseg.FusedVNDGCNNPSeg
that need no device.  The kernels themselves: tests/test_hip_vn_pseg.py."""
import argparse
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import vn_cases as VC
from tests import vn_pseg_cases as PC
from tests import vn_pseg_ref as P
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import compare_case

F32 = np.float32
GOLDEN = PC.GOLDEN


def test_reference_state_loads_strictly_and_the_model_reproduces_the_recorded_run():
    """The reference's state_dict layout loads with strict=True, and the model on the recorded lists reproduces the recorded levels,
    conv8's input and the logits.  Worst values found while writing this (torch on the CPU, the reference's own operations): 0 for
    every key."""
    import svnet_amd.models as M
    seed, B, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model()
    assert isinstance(model, M.VN_DGCNN_PSEG) and list(model.state_dict()) == [str(key) for key in GOLDEN["keys"]]
    assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(int(d) for d in s if d >= 0) for s in GOLDEN["shapes"]]
    assert model.conv8[1] is model.bn8 and model.conv7[1] is model.bn7 and model.conv9[1] is model.bn9 and model.conv10[1] is model.bn10
    levels = model.edge_levels()
    assert [len(convs) for convs, _ in levels] == [2, 2, 1] and levels[0][0] == (model.conv1, model.conv2) and levels[2][0] == (model.conv5,)
    x, l = torch.from_numpy(GOLDEN["x"]), torch.from_numpy(GOLDEN["l"])
    assert sorted(int(c) for c in GOLDEN["l"].argmax(1)) == sorted(P.GOLDEN_LABELS) and (GOLDEN["l"].sum(1) == 1).all()
    lists = [torch.from_numpy(i) for i in PC.lists()]
    seen = []
    hook = model.conv8.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
    from svnet_amd.models.utils.vn_util import get_graph_feature
    with torch.no_grad():
        logits = model(x, l, idx=lists)
        h, feats = x.unsqueeze(1), []
        for i, (convs, pool) in enumerate(levels):
            h = get_graph_feature(h, k=k, idx=lists[i])
            for conv in convs:
                h = conv(h)
            h = pool(h)
            feats.append(h)
        assert torch.equal(model.tail(feats, l), logits)
    hook.remove()
    head = seen[0].numpy()
    got = {"out:lvl%d" % i: f.numpy() for i, f in enumerate(feats)}
    got.update({"out:g_max": head[:, :P.POOLED, 0], "out:label64": head[:, P.POOLED:P.POOLED + P.LABEL, 0], "out:coords": head[:, P.POOLED + P.LABEL:],
                "out:logits": logits.numpy()})
    assert tuple(logits.shape) == (B, num_part, N) and head.shape == (B, P.POOLED + P.LABEL + P.COORDS, N)
    worst = compare_case(got, {key: GOLDEN[key[4:]] for key in got}, 1e-3, "the model against the recorded run")
    print("worst relative error %.3e at %s" % worst)
    with pytest.raises(ValueError, match="three levels"):
        model(x, l, idx=lists[:2])


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_model_constructs_and_runs_in_both_poolings_and_in_train_mode(pooling):
    import svnet_amd.models as M
    B, N, k, num_part = 2, 12, 4, 7
    torch.manual_seed(3)
    model = M.VN_DGCNN_PSEG(argparse.Namespace(k=k, pooling=pooling), num_part)
    assert ("pool1.map_to_dir.weight" in model.state_dict()) == (pooling == "max")
    x = torch.from_numpy(synth.cloud_batch(3, 0, 0, B, N))
    l = torch.from_numpy(synth.category_onehot(3, 0, 0, B))
    lists = [torch.from_numpy(synth.integers(3, i, (B, N, k), N)) for i in range(3)]
    model.train()
    out = model(x, l, idx=lists)
    assert tuple(out.shape) == (B, num_part, N) and out.requires_grad and bool(torch.isfinite(out).all())
    out.square().mean().backward()
    # (a VNMaxPool's direction only selects: it takes no gradient)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for name, p in model.named_parameters() if not name.startswith("pool"))
    assert int(model.bn8.num_batches_tracked) == 1 and int(model.conv2.batchnorm.bn.num_batches_tracked) == 1
    model.eval()
    with torch.no_grad():
        a, b = model(x, l, idx=lists), model(x, l, idx=lists)
    assert torch.equal(a, b) and tuple(a.shape) == (B, num_part, N)
    with pytest.raises(ValueError, match="pooling"):
        M.VN_DGCNN_PSEG(argparse.Namespace(k=k, pooling="sum"))


def test_restatement_equals_the_recorded_levels_and_coordinates():
    st = PC.state()
    seed, B, N, k, num_part = P.GOLDEN_CASE
    h = GOLDEN["x"][:, None]
    for i, (prefixes, widths) in enumerate(zip(P.LEVEL_PREFIXES, P.LEVEL_WIDTHS)):
        f1 = V.fold_state(st, prefixes[0])
        assert h.shape == (B, widths[0], 3, N)
        if len(prefixes) == 2:
            got = P.level2_batch(h, GOLDEN["idx%d" % i], f1, T.fold_point_state(st, prefixes[1]))
        else:
            got = V.level_batch(h, GOLDEN["idx%d" % i], f1)
        assert got.dtype == F32 and got.shape == (B, widths[-1], 3, N)
        worst = compare_case({"out": got}, {"out": GOLDEN["lvl%d" % i]}, 1e-3, "level %d against the recorded one" % i)
        print("level %d: worst relative error %.3e" % (i, worst[0]))
        h = GOLDEN["lvl%d" % i]
    x123, y = PC.frame_inputs()
    coords = np.stack([P.std_coords(x123[b], y[b], st["std_feature.vn_lin.weight"]) for b in range(B)])
    assert coords.dtype == F32 and coords.shape == (B, P.COORDS, N)
    compare_case({"out": coords}, {"out": GOLDEN["coords"]}, 1e-3, "the coordinates against the recorded ones")
    # the pooled half of conv8's input is the maximum over the points of the same rules on [local | its mean]
    f6 = T.fold_point_state(st, "conv6.")
    local = T.point_level(x123[0], f6)
    pooled = T.std_pool(local, y[0], st["std_feature.vn_lin.weight"], g=T.ordered_mean(local))[:P.POOLED]
    compare_case({"out": pooled}, {"out": GOLDEN["g_max"][0]}, 1e-3, "the pooled features against the recorded ones")


@pytest.mark.parametrize("C,O1,O2,N,k,share1,share2,slope", [(2, 3, 5, 17, 1, False, False, 0.2), (4, 6, 7, 33, 17, True, False, 0.2),
                                                             (5, 1, 1, 1, 1, False, False, 0.2), (3, 20, 9, 20, 4, True, True, 0.0)])
def test_restatement_against_float64_and_the_modules(C, O1, O2, N, k, share1, share2, slope):
    seed = 60 + C
    x, idx = synth.normal(seed, 1, (C, 3, N)), synth.integers(seed, 2, (N, k), 3 * N) - N
    a1, a2 = VC.layer_arrays(seed, 2 * C, O1, 1 if share1 else O1), VC.layer_arrays(seed + 1, O1, O2, 1 if share2 else O2)
    keys = ("w_feat", "w_dir", "gamma", "beta", "mean", "var")
    taken = []
    got = P.level2(x, idx, V.fold(*(a1[key] for key in keys)), T.fold_point(*(a2[key] for key in keys)), slope, slope, taken)
    assert got.dtype == F32 and got.shape == (O2, 3, N) and len(taken) == 1 and all(0 <= s <= 1 for s in taken[0])
    compare_case({"out": got}, {"out": P.level2_f64(x, idx, a1, a2, slope, slope)}, 1e-3, "against the float64 direct form")
    from svnet_amd.models.utils.vn_util import get_graph_feature
    l1, l2 = VC.layer(None, 2 * C, O1, share1, slope, a1), VC.layer(None, O1, O2, share2, slope, a2)
    with torch.no_grad():
        mod = l2(l1(get_graph_feature(torch.from_numpy(x)[None], k=k, idx=torch.from_numpy(idx).clamp(0, N - 1)[None]))).mean(dim=-1)[0]
    compare_case({"out": got}, {"out": mod.numpy()}, 1e-3, "against the modules")
    # the coordinates against the einsum in float64
    y, w_lin = synth.normal(seed, 3, (O2, 3, N)), synth.normal(seed, 4, (3, O2))
    e = P.std_coords(got, y, w_lin)
    assert e.dtype == F32 and e.shape == (3 * O2, N)
    compare_case({"out": e}, {"out": P.std_coords_f64(got, y, w_lin)}, 1e-3, "coordinates against float64")
    assert np.array_equal(e.max(axis=1), T.std_pool(got, y, w_lin)[:3 * O2])


def test_header_names_the_entries_under_abi_434():
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 434
    names = ("svnet_vn_edge2_supported", "svnet_vn_edge2_mean_f32", "svnet_vn_std_coords_supported", "svnet_vn_std_coords_f32")
    assert "434: " + ", ".join(names) in header and "433: svnet_vn_point_supported" in header
    assert "fused two-layer vector-neuron edge level" in header and "frame coordinates per point" in header
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_vn_edge2_mean_f32"][1][13] is _lib.c_f and _lib.SIGNATURES["svnet_vn_edge2_mean_f32"][1][14] is _lib.c_f
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    # both sides of every edge of the envelope: (N, k, C, O1, Od1, O2, Od2)
    S = VF.supported2
    assert not S(64, 0, 4, 4, 4, 4, 4) and S(64, 1, 4, 4, 4, 4, 4) and S(64, 64, 4, 4, 4, 4, 4) and not S(128, 65, 4, 4, 4, 4, 4)
    assert not S(7, 8, 4, 4, 4, 4, 4) and S(8, 8, 4, 4, 4, 4, 4) and S(32768, 8, 4, 4, 4, 4, 4) and not S(32769, 8, 4, 4, 4, 4, 4)
    assert not S(64, 8, 0, 4, 4, 4, 4) and S(64, 8, 1, 4, 4, 4, 4) and S(64, 8, 128, 4, 4, 4, 4) and not S(64, 8, 129, 4, 4, 4, 4)
    assert not S(64, 8, 4, 0, 0, 4, 4) and S(64, 8, 4, 1, 1, 4, 4) and S(64, 8, 4, 128, 128, 4, 4) and not S(64, 8, 4, 129, 129, 4, 4)
    assert not S(64, 8, 4, 4, 4, 0, 0) and S(64, 8, 4, 4, 4, 1, 1) and S(64, 8, 4, 4, 4, 128, 128) and not S(64, 8, 4, 4, 4, 129, 129)
    assert S(64, 8, 4, 7, 1, 9, 1) and S(64, 8, 4, 128, 1, 128, 1) and S(64, 64, 128, 128, 128, 128, 128)
    assert not S(64, 8, 4, 7, 2, 9, 9) and not S(64, 8, 4, 7, 0, 9, 9) and not S(64, 8, 4, 7, 7, 9, 2) and not S(64, 8, 4, 7, 7, 9, 0)
    assert all(S(2048, 40, w[0], w[1], w[1], w[2], w[2]) for w in P.LEVEL_WIDTHS[:2])
    K = VT.supported_coords                                                       # (N, C, Cy)
    assert not K(0, 4, 4) and K(1, 4, 4) and K(32768, 4, 4) and not K(32769, 4, 4)
    assert not K(16, 0, 4) and K(16, 1, 1) and K(16, 512, 512) and not K(16, 513, 4) and not K(16, 4, 0) and not K(16, 4, 513)
    assert K(2048, 63, 170)
    L = _lib.lib()
    p = _lib.c_p(64)                                                              # refused before any launch: no device is touched
    E = _lib.DEFINES
    assert L.svnet_vn_edge2_mean_f32(None, 1 << 30, p, p, p, 1, 64, 8, 4, 4, 4, 4, 4, 0.2, 0.2, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge2_mean_f32(p, 1 << 30, p, p, None, 1, 64, 8, 4, 4, 4, 4, 4, 0.2, 0.2, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge2_mean_f32(p, 1 << 30, p, p, p, 0, 64, 8, 4, 4, 4, 4, 4, 0.2, 0.2, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge2_mean_f32(p, 1 << 30, p, p, p, 1, 64, 65, 4, 4, 4, 4, 4, 0.2, 0.2, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_edge2_mean_f32(p, 1 << 30, p, p, p, 1, 64, 8, 4, 4, 4, 129, 129, 0.2, 0.2, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_edge2_mean_f32(p, 16, p, p, p, 1, 64, 8, 4, 4, 4, 4, 4, 0.2, 0.2, p, None) == E["SVNET_E_WORKSPACE"]
    assert b"svnet_vn_edge2_mean_f32" in L.svnet_last_error()
    assert L.svnet_vn_std_coords_f32(p, None, p, 1, 16, 4, 4, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_std_coords_f32(p, p, p, 65536, 16, 4, 4, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_std_coords_f32(p, p, p, 1, 16, 513, 4, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_std_coords_f32" in L.svnet_last_error()


_fake = VC.fake


def test_fronts_refuse_bad_arguments_before_any_device_call():
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    B, C, N, k, O1, O2, Cy = 2, 3, 16, 4, 5, 6, 4
    x, idx = torch.zeros(B, C, 3, N), torch.zeros(B, N, k, dtype=torch.int64)
    f1 = _fake(VF.FoldedVNLayer, C=C, O=O1, Od=O1)
    f2 = _fake(VT.FoldedVNPoint, C=O1, Cg=0, O=O2, Od=O2)
    with pytest.raises(TypeError, match="folded1 must be a FoldedVNLayer"):
        VF.vn_edge2_mean(x, idx, f2, f2)
    with pytest.raises(TypeError, match="folded2 must be a FoldedVNPoint"):
        VF.vn_edge2_mean(x, idx, f1, f1)
    with pytest.raises(TypeError, match="x must be torch.float32"):
        VF.vn_edge2_mean(x.double(), idx, f1, f2)
    with pytest.raises(TypeError, match="idx must be torch.int64"):
        VF.vn_edge2_mean(x, idx.int(), f1, f2)
    with pytest.raises(ValueError, match="x requires grad"):
        VF.vn_edge2_mean(x.clone().requires_grad_(), idx, f1, f2)
    with pytest.raises(ValueError, match="x must be contiguous"):
        VF.vn_edge2_mean(torch.zeros(B, C, N, 3).transpose(2, 3), idx, f1, f2)
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VF.vn_edge2_mean(torch.zeros(B, C, N), idx, f1, f2)
    with pytest.raises(ValueError, match=r"idx must be \[B,N,k\]"):
        VF.vn_edge2_mean(x, idx[:, :8].contiguous(), f1, f2)
    with pytest.raises(ValueError, match="the first layer takes 4 vector channels"):
        VF.vn_edge2_mean(x, idx, _fake(VF.FoldedVNLayer, C=4, O=O1, Od=O1), f2)
    with pytest.raises(ValueError, match="the second layer must take the first one's 5 channels"):
        VF.vn_edge2_mean(x, idx, f1, _fake(VT.FoldedVNPoint, C=O1 + 1, Cg=0, O=O2, Od=O2))
    with pytest.raises(ValueError, match="no constant ones"):
        VF.vn_edge2_mean(x, idx, f1, _fake(VT.FoldedVNPoint, C=O1, Cg=2, O=O2, Od=O2))
    with pytest.raises(ValueError, match="out must be"):
        VF.vn_edge2_mean(x, idx, f1, f2, out=torch.zeros(B, O1, 3, N))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # everything in order but the device
        VF.vn_edge2_mean(x, idx, f1, f2, out=torch.zeros(B, O2, 3, N))
    y, w = torch.zeros(B, Cy, 3, N), torch.zeros(3, Cy)
    with pytest.raises(TypeError, match="w_lin must be torch.float32"):
        VT.vn_std_coords(x, y, w.double())
    with pytest.raises(ValueError, match="y requires grad"):
        VT.vn_std_coords(x, y.clone().requires_grad_(), w)
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VT.vn_std_coords(torch.zeros(B, C, N), y, w)
    with pytest.raises(ValueError, match=r"y must be \[B,Cy,3,N\]"):
        VT.vn_std_coords(x, torch.zeros(B, Cy, 3, N + 1), w)
    with pytest.raises(ValueError, match=r"w_lin must be \[3,Cy\]"):
        VT.vn_std_coords(x, y, torch.zeros(2, Cy))
    with pytest.raises(ValueError, match="out must be"):
        VT.vn_std_coords(x, y, w, out=torch.zeros(B, C, 3, N))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.vn_std_coords(x, y, w, out=torch.zeros(B, 3 * C, N))


def test_wrapper_refuses_what_it_cannot_take():
    from svnet_amd import vn_pseg as VP
    with pytest.raises(TypeError, match="VN_DGCNN_PSEG"):
        VP.FusedVNDGCNNPSeg(VC.golden_model())                                    # (the classifier)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VP.FusedVNDGCNNPSeg(PC.golden_model())
    # pooling = 'max' and normalize_frame: nothing to fold, so the wrapper lives on the CPU too; every call is the model's
    for model in (PC.golden_model(pooling="max"), PC.golden_model()):
        model.std_feature.normalize_frame = True
        fused = VP.FusedVNDGCNNPSeg(model)
        assert not fused.fused and not fused.levels and not fused.points and not fused.supported(2, 64, 8)
        x, l, lists = torch.from_numpy(GOLDEN["x"]), torch.from_numpy(GOLDEN["l"]), [torch.from_numpy(i) for i in PC.lists()]
        VC.cpu_wrapper_refuses(fused, (x, l), [
            (TypeError, "x must be torch.float32", (x.double(), l), {}),
            (ValueError, "l requires grad", (x, l.clone().requires_grad_()), {}),
            (ValueError, r"x must be \[B,3,N\]", (x[:, :2].contiguous(), l), {}),
            (ValueError, r"l must be \[B,16\]", (x, l[:1].contiguous()), {}),
            (ValueError, "three levels", (x, l), {"idx": lists[:2]}),
            (RuntimeError, "no CPU fallback", (x, l), {"idx": lists})])
