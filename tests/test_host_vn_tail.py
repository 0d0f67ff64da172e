"""CPU tests of the fused vector-neuron tail: the numpy restatement tests/vn_tail_ref.py against the reference's recorded run
(tests/golden/vn.npz), the module's own tail and float64 direct forms; the algebra of the cloud term; the header's new entry points;
and the refusals of svnet_amd/vn_tail.py that need no device.  The kernels themselves: tests/test_hip_vn_tail.py."""
import functools
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import vn_cases as VC
from tests import vn_ref as V
from tests import vn_tail_ref as T
from tests.common import compare_case

F32 = np.float32
GOLDEN = VC.GOLDEN
golden_state, golden_model = VC.state, functools.partial(VC.golden_model, None)


def head(model, h):
    """The head through the model's own modules, as FusedVNTail runs it."""
    with torch.no_grad():
        h = torch.from_numpy(h)
        for layer in (1, 2):
            linear, bn, drop = (getattr(model, "%s%d" % (n, layer)) for n in ("linear", "bn", "dp"))
            h = drop(torch.nn.functional.leaky_relu(bn(linear(h)), negative_slope=0.2))
        return model.linear3(h).numpy()


def test_restatement_of_the_tail_equals_the_recorded_logits_and_the_module():
    """The whole tail restated on the four recorded level outputs: against the recorded logits and against model.tail on the CPU."""
    model = golden_model()
    levels = [GOLDEN["lvl%d" % i] for i in range(4)]
    h = T.pooled(levels, golden_state())
    assert h.shape == (V.GOLDEN_CASE[1], 6 * 682) and h.dtype == F32 and np.isfinite(h).all()
    logits = head(model, h)
    with torch.no_grad():
        mod = model.tail([torch.from_numpy(l) for l in levels]).numpy()
    w_ref = compare_case({"out:logits": logits}, {"out:logits": GOLDEN["logits"]}, 1e-3, "against the recorded logits")
    w_mod = compare_case({"out:logits": logits}, {"out:logits": mod}, 1e-3, "against model.tail")
    print("worst relative error %.3e against the recorded logits, %.3e against model.tail" % (w_ref[0], w_mod[0]))


def _arrays(C, Cg, O, Od, N, seed):
    return dict(VC.layer_arrays(seed, C + Cg, O, Od), x=synth.normal(seed, 1, (C, 3, N)), g=synth.normal(seed, 2, (Cg, 3)))


@pytest.mark.parametrize("C,Cg,O,Od,N,slope", [(5, 0, 7, 7, 9, 0.2), (3, 2, 70, 1, 20, 0.0), (6, 5, 20, 20, 33, 0.2), (40, 40, 12, 12, 70, 0.2)])
def test_point_level_against_float64_and_the_expanded_input(C, Cg, O, Od, N, slope):
    a = _arrays(C, Cg, O, Od, N, 70 + C)
    f = T.fold_point(a["w_feat"], a["w_dir"], a["gamma"], a["beta"], a["mean"], a["var"])
    got = T.point_level(a["x"], f, slope, a["g"] if Cg else None)
    full = T.expanded(a["x"], a["g"]) if Cg else a["x"]
    want = T.point_level_f64(full, a["w_feat"], a["w_dir"], a["gamma"], a["beta"], a["mean"], a["var"], slope=slope)
    assert got.dtype == F32 and got.shape == want.shape == (O, 3, N)
    compare_case({"out": got}, {"out": want}, 1e-3, "against the float64 direct form")
    if Cg:
        # the algebra of the saving: the chain that starts at the cloud term against the same layer on the explicitly expanded input
        direct = T.point_level(full, f, slope)
        worst = compare_case({"out": got}, {"out": direct}, 1e-3, "against the expanded [x | g] input")
        assert worst[0] > 0 or C + Cg < 8                                         # the two orders differ in rounding, and only in rounding


@pytest.mark.parametrize("N", [1, 64, 65, 130])
def test_cloud_mean_and_std_pool_against_float64(N):
    C, Cg, Cy = 5, 5, 3
    x, g = synth.normal(80 + N, 1, (C, 3, N)), synth.normal(80 + N, 2, (Cg, 3))
    y, w_lin = synth.normal(80 + N, 3, (Cy, 3, N)), synth.normal(80 + N, 4, (3, Cy))
    m = T.ordered_mean(x)
    assert m.dtype == F32 and m.shape == (C, 3)
    compare_case({"out": m}, {"out": x.astype(np.float64).mean(-1)}, 1e-3, "cloud mean")
    if N <= 64:                                                                    # one run: the plain n-ascending sum
        s = np.zeros((C, 3), dtype=F32)
        for n in range(N):
            s = (s + x[..., n]).astype(F32)
        assert np.array_equal(m, (s / F32(N)).astype(F32))
    h = T.std_pool(x, y, w_lin, g)
    assert h.dtype == F32 and h.shape == (6 * (C + Cg),)
    compare_case({"out": h}, {"out": T.std_pool_f64(T.expanded(x, g), y, w_lin)}, 1e-3, "std-pool")
    compare_case({"out": T.std_pool(x, y, w_lin)}, {"out": T.std_pool_f64(x, y, w_lin)}, 1e-3, "std-pool without constant channels")
    # against the module: VNStdFeature's einsum on the frame, then [amax | mean]
    from svnet_amd.models.vn_layers import _channels_last
    lin = torch.nn.Linear(Cy, 3, bias=False)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w_lin))
        frame = _channels_last(lin, torch.from_numpy(y)[None]).transpose(1, 2)
        inv = torch.einsum('bij...,bjk...->bik...', torch.from_numpy(T.expanded(x, g))[None], frame).flatten(1, 2)
        mod = torch.cat((inv.amax(dim=-1), inv.mean(dim=-1)), dim=1)[0].numpy()
    compare_case({"out": h}, {"out": mod}, 1e-3, "std-pool against the module's einsum")


def test_header_names_the_tail_entries_under_abi_433():
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 433
    names = ("svnet_vn_point_supported", "svnet_vn_point_workspace_bytes", "svnet_vn_point_fold_f32", "svnet_vn_point_f32", "svnet_vn_cloud_mean_f32",
             "svnet_vn_std_pool_supported", "svnet_vn_std_pool_workspace_bytes", "svnet_vn_std_pool_f32")
    assert "433: " + ", ".join(names) in header and "fused vector-neuron tail for inference" in header
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_vn_point_workspace_bytes"][0] is _lib.c_sz and _lib.SIGNATURES["svnet_vn_point_f32"][1][9] is _lib.c_f
    from svnet_amd import vn_tail as VT
    # both sides of every edge of the envelope
    P, S = VT.supported_point, VT.supported_std
    assert not P(0, 4, 0, 4, 4) and P(1, 4, 0, 4, 4) and P(32768, 4, 0, 4, 4) and not P(32769, 4, 0, 4, 4)
    assert not P(16, 0, 0, 4, 4) and P(16, 1, 0, 4, 4) and P(16, 512, 0, 4, 4) and not P(16, 513, 0, 4, 4)
    assert not P(16, 4, -1, 4, 4) and P(16, 4, 512, 4, 4) and not P(16, 4, 513, 4, 4)
    assert not P(16, 4, 0, 0, 0) and P(16, 4, 0, 1, 1) and P(16, 4, 0, 512, 512) and not P(16, 4, 0, 513, 513)
    assert P(16, 4, 0, 7, 1) and not P(16, 4, 0, 7, 2) and not P(16, 4, 0, 7, 0)
    assert not S(0, 4, 0, 4) and S(1, 4, 0, 4) and S(32768, 4, 0, 4) and not S(32769, 4, 0, 4)
    assert not S(16, 0, 0, 4) and S(16, 512, 512, 512) and not S(16, 513, 0, 4) and not S(16, 4, 513, 4) and not S(16, 4, -1, 4)
    assert not S(16, 4, 0, 0) and not S(16, 4, 0, 513)
    assert all(P(1024, *w) for w in T.MODEL_POINT) and S(1024, *T.MODEL_STD)
    L = _lib.lib()
    assert L.svnet_vn_point_workspace_bytes(32, 341, 341, 341) == 32 * 3 * 682 * 4 and L.svnet_vn_point_workspace_bytes(3, 2, 70, 1) == 3 * 3 * 71 * 4
    assert L.svnet_vn_point_workspace_bytes(32, 0, 341, 1) == 0 and L.svnet_vn_point_workspace_bytes(0, 2, 4, 4) == 0
    assert L.svnet_vn_point_workspace_bytes(65536, 2, 4, 4) == 0 and L.svnet_vn_point_workspace_bytes(2, 2, 513, 513) == 0
    assert L.svnet_vn_std_pool_workspace_bytes(32, 1024, 341, 341) == 2 * 16 * 32 * 3 * 682 * 4
    assert L.svnet_vn_std_pool_workspace_bytes(2, 65, 5, 5) == 2 * 2 * 2 * 30 * 4 and L.svnet_vn_std_pool_workspace_bytes(2, 64, 4, 0) == 2 * 2 * 12 * 4
    assert L.svnet_vn_std_pool_workspace_bytes(0, 64, 4, 0) == 0 and L.svnet_vn_std_pool_workspace_bytes(2, 64, 513, 0) == 0
    p = _lib.c_p(64)                                                              # refused before any launch: no device is touched
    E = _lib.DEFINES
    assert L.svnet_vn_point_fold_f32(None, p, p, p, p, p, 4, 0, 4, 4, 1e-5, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_point_fold_f32(p, p, p, p, p, p, 4, 0, 4, 2, 1e-5, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_point_fold_f32" in L.svnet_last_error()
    assert L.svnet_vn_point_f32(None, None, p, 1, 16, 4, 0, 4, 4, 0.2, None, 0, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_point_f32(p, None, p, 1, 16, 4, 2, 4, 4, 0.2, p, 1 << 20, p, None) == E["SVNET_E_ARG"]          # g missing with Cg > 0
    assert L.svnet_vn_point_f32(p, p, p, 65536, 16, 4, 2, 4, 4, 0.2, p, 1 << 40, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_point_f32(p, p, p, 1, 32769, 4, 2, 4, 4, 0.2, p, 1 << 20, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_point_f32(p, p, p, 1, 16, 4, 2, 4, 4, 0.2, p, 16, p, None) == E["SVNET_E_WORKSPACE"]
    assert b"svnet_vn_point_f32" in L.svnet_last_error()
    assert L.svnet_vn_cloud_mean_f32(p, 1, 4, 16, None, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_cloud_mean_f32(p, 0, 4, 16, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_cloud_mean_f32(p, 1, 513, 16, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_cloud_mean_f32" in L.svnet_last_error()
    assert L.svnet_vn_std_pool_f32(p, None, None, p, 1, 16, 4, 0, 4, p, 1 << 20, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_std_pool_f32(p, None, p, p, 1, 16, 4, 2, 4, p, 1 << 20, p, None) == E["SVNET_E_ARG"]             # g missing with Cg > 0
    assert L.svnet_vn_std_pool_f32(p, p, p, p, 1, 16, 4, 2, 513, p, 1 << 20, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_std_pool_f32(p, p, p, p, 1, 16, 4, 2, 4, p, 16, p, None) == E["SVNET_E_WORKSPACE"]
    assert b"svnet_vn_std_pool_f32" in L.svnet_last_error()


def _fake_folded(C, Cg, O, Od=None):
    from svnet_amd import vn_tail as VT
    return VC.fake(VT.FoldedVNPoint, C=C, Cg=Cg, O=O, Od=O if Od is None else Od)


def test_front_refuses_bad_arguments():
    from svnet_amd import vn_tail as VT
    B, C, Cg, N, O, Cy = 2, 3, 2, 16, 5, 4
    x, g, f = torch.zeros(B, C, 3, N), torch.zeros(B, Cg, 3), _fake_folded(C, Cg, O)
    with pytest.raises(TypeError, match="FoldedVNPoint"):
        VT.vn_point(x, object())
    with pytest.raises(TypeError, match="x must be torch.float32"):
        VT.vn_point(x.double(), f, cloud=g)
    with pytest.raises(TypeError, match="cloud must be a tensor"):
        VT.vn_point(x, f, cloud=g.numpy())
    with pytest.raises(ValueError, match="x requires grad"):
        VT.vn_point(x.clone().requires_grad_(), f, cloud=g)
    with pytest.raises(ValueError, match="cloud requires grad"):
        VT.vn_point(x, f, cloud=g.clone().requires_grad_())
    with pytest.raises(ValueError, match="x must be contiguous"):
        VT.vn_point(torch.zeros(B, C, N, 3).transpose(2, 3), f, cloud=g)
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VT.vn_point(torch.zeros(B, C, N), f, cloud=g)
    with pytest.raises(ValueError, match="the layer takes 4 vector channels"):
        VT.vn_point(x, _fake_folded(4, Cg, O), cloud=g)
    with pytest.raises(ValueError, match=r"cloud must be \[B,Cg,3\]"):
        VT.vn_point(x, f)
    with pytest.raises(ValueError, match=r"cloud must be \[B,Cg,3\]"):
        VT.vn_point(x, f, cloud=torch.zeros(B, Cg + 1, 3))
    with pytest.raises(ValueError, match=r"cloud must be \[B,Cg,3\]"):
        VT.vn_point(x, _fake_folded(C, 0, O), cloud=g)
    with pytest.raises(ValueError, match="out must be"):
        VT.vn_point(x, f, cloud=g, out=torch.zeros(B, O, N, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # everything in order but the device
        VT.vn_point(x, f, cloud=g, out=torch.zeros(B, O, 3, N))
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VT.vn_cloud_mean(torch.zeros(B, C, N))
    with pytest.raises(ValueError, match="out must be"):
        VT.vn_cloud_mean(x, out=torch.zeros(B, C))
    with pytest.raises(ValueError, match="x requires grad"):
        VT.vn_cloud_mean(x.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.vn_cloud_mean(x)
    y, w = torch.zeros(B, Cy, 3, N), torch.zeros(3, Cy)
    with pytest.raises(TypeError, match="w_lin must be torch.float32"):
        VT.vn_std_pool(x, y, w.double())
    with pytest.raises(ValueError, match=r"y must be \[B,Cy,3,N\]"):
        VT.vn_std_pool(x, torch.zeros(B, Cy, 3, N + 1), w)
    with pytest.raises(ValueError, match=r"w_lin must be \[3,Cy\]"):
        VT.vn_std_pool(x, y, torch.zeros(2, Cy))
    with pytest.raises(ValueError, match=r"cloud must be \[B,Cg,3\]"):
        VT.vn_std_pool(x, y, w, cloud=torch.zeros(B + 1, Cg, 3))
    with pytest.raises(ValueError, match="out must be"):
        VT.vn_std_pool(x, y, w, cloud=g, out=torch.zeros(B, 6 * C))
    with pytest.raises(ValueError, match="y requires grad"):
        VT.vn_std_pool(x, y.clone().requires_grad_(), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.vn_std_pool(x, y, w, cloud=g)


def test_fold_and_wrappers_refuse_what_they_cannot_take():
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    from svnet_amd.models import vn_layers as L
    with pytest.raises(TypeError, match="VNLinearLeakyReLU"):
        VT.fold_vn_point(L.VNLinear(4, 4))
    with pytest.raises(ValueError, match="cloud_channels"):
        VT.fold_vn_point(L.VNLinearLeakyReLU(4, 4, dim=4), cloud_channels=4)
    with pytest.raises(ValueError, match="cloud_channels"):
        VT.fold_vn_point(L.VNLinearLeakyReLU(4, 4, dim=4), cloud_channels=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.fold_vn_point(L.VNLinearLeakyReLU(5, 4, dim=4), cloud_channels=2)
    with pytest.raises(TypeError, match="VN_DGCNN_CLS"):
        VT.FusedVNTail(torch.nn.Linear(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.FusedVNTail(golden_model())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.FusedVNDGCNN(golden_model(), tail=True)
    # normalize_frame: nothing to fold, so the wrapper lives on the CPU too; every call is model.tail's
    model = golden_model()
    model.std_feature.normalize_frame = True
    tail = VT.FusedVNTail(model)
    assert not tail.fused and not tail.supported(2, 64)
    feats = [torch.from_numpy(GOLDEN["lvl%d" % i]) for i in range(4)]
    VC.cpu_wrapper_refuses(tail, (feats,), [
        (TypeError, r"feats\[0\] must be torch.float32", ([f.double() for f in feats],), {}),
        (ValueError, r"feats\[2\] requires grad", ([f.clone().requires_grad_() if i == 2 else f for i, f in enumerate(feats)],), {}),
        (ValueError, r"feats must be \[B,C_i,3,N\]", ([feats[0], feats[1][:, :, :, :8].contiguous()],), {}),
        (ValueError, "feats must hold", ([],), {}),
        (RuntimeError, "no CPU fallback", (feats,), {})])
    # pooling = 'max' with tail=True: no tail is built, as no level is
    fused = VF.FusedVNDGCNN(golden_model("max"), tail=True)
    assert fused.tail is None and not fused.levels and fused.refresh() is fused and fused.release() is fused
    ws = VT._Workspace(torch.device("cpu"))
    first = ws.take(8)
    assert ws.take(4) is first and ws.take(16) is not first and ws._retired == [first]
    ws.release()
    assert ws._retired == []
