"""CPU tests of the vector-neuron PointNet path: the torch model svnet_amd.models.VN_PointNet_CLS against the reference's recorded run
(tests/golden/vn_pointnet.npz), the numpy restatement tests/vn_pointnet_ref.py against the same recordings and its float64 formulas,
the header's new entry points, and the refusals of vn_pointnet.vn_edge_cross_mean, vn_tail.vn_point_norm and
vn_pointnet.FusedVNPointNet that need no device.  The kernels themselves: tests/test_hip_vn_pointnet.py."""
import argparse
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import vn_cases as VC
from tests import vn_pointnet_cases as PC
from tests import vn_pointnet_ref as P
from tests.common import compare_case

F32 = np.float32
GOLDEN = PC.GOLDEN


def _model_stages(model, x, idx):
    """{stage: array} of the module's forward on the list idx, by the model's own accessors."""
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross
    enc = model.feat
    with torch.no_grad():
        logits = model(x, idx=idx)
        conv_pos, pool = enc.position_level()
        pos = pool(conv_pos(get_graph_feature_cross(x.unsqueeze(1), k=model.k, idx=idx)))
        x1 = enc.conv1(pos)
        g = enc.fstn(x1)
        x2 = enc.conv2(torch.cat((x1, g.unsqueeze(-1).expand(-1, -1, -1, x1.size(-1))), dim=1))
        h = enc.pooled(enc.local_feature(pos))
        assert torch.equal(model.head(h), logits) and torch.equal(enc(x, idx=idx), h)
    return {"out:pos": pos.numpy(), "out:conv1": x1.numpy(), "out:fstn": g.numpy(), "out:conv2": x2.numpy(), "out:h": h.numpy(),
            "out:logits": logits.numpy()}


def test_reference_state_loads_strictly_and_the_model_reproduces_the_recorded_run():
    """The reference's state_dict layout loads with strict=True, and the model on the recorded list reproduces every recorded stage and
    the logits within the project's tolerance (torch.cross on an expanded view need not round as the reference's does, so bit equality
    is not asked).  Worst value found while writing this (torch on the CPU): 0 for every key."""
    import svnet_amd.models as M
    seed, B, N, k, num_class = P.GOLDEN_CASE
    model = PC.golden_model()
    assert isinstance(model, M.VN_PointNet_CLS) and list(model.state_dict()) == [str(key) for key in GOLDEN["keys"]]
    assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(int(d) for d in s if d >= 0) for s in GOLDEN["shapes"]]
    assert model.k == k and len(model.feat.fstn.point_layers()) == 3
    got = _model_stages(model, torch.from_numpy(GOLDEN["x"]), torch.from_numpy(GOLDEN["idx"]))
    assert sorted(got) == sorted("out:" + key for key in P.STAGES) and got["out:logits"].shape == (B, num_class)
    worst = compare_case(got, {key: GOLDEN[key[4:]] for key in got}, 1e-3, "the model against the recorded run")
    print("worst relative error %.3e at %s" % worst)
    with pytest.raises(ValueError, match="one neighbour list"):
        model(torch.from_numpy(GOLDEN["x"]), idx=[torch.from_numpy(GOLDEN["idx"])])


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_model_and_stnkd_construct_and_run_in_both_poolings_and_in_train_mode(pooling):
    import svnet_amd.models as M
    from svnet_amd.models.vn_layers import STNkd, VNMaxPool
    B, N, k, num_class = 2, 12, 4, 5
    torch.manual_seed(3)
    args = argparse.Namespace(k=k, pooling=pooling)
    stn = STNkd(args, d=6)
    assert isinstance(stn.pool, VNMaxPool) == (pooling == "max") and stn.d == 6
    assert [key.split(".")[0] for key in stn.state_dict() if key.endswith("map_to_feat.weight")] == ["conv1", "conv2", "conv3", "fc1", "fc2", "fc3"]
    with torch.no_grad():
        t = stn.eval()(torch.from_numpy(synth.normal(3, 1, (B, 6, 3, N))))
    assert tuple(t.shape) == (B, 6, 3) and bool(torch.isfinite(t).all())
    model = M.VN_PointNet_CLS(args, num_class)
    keys = list(model.state_dict())
    assert ("feat.pool.map_to_dir.weight" in keys) == ("feat.fstn.pool.map_to_dir.weight" in keys) == (pooling == "max")
    x = torch.from_numpy(synth.cloud_batch(3, 0, 0, B, N))
    idx = torch.from_numpy(synth.integers(3, 1, (B, N, k), N))
    model.train()
    out = model(x, idx=idx)
    assert tuple(out.shape) == (B, num_class) and out.requires_grad and bool(torch.isfinite(out).all())
    out.square().mean().backward()
    # (a VNMaxPool's direction only selects: it takes no gradient)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for name, p in model.named_parameters() if ".pool." not in name)
    assert int(model.bn1.num_batches_tracked) == 1 and int(model.feat.bn3.bn.num_batches_tracked) == 1
    model.eval()
    with torch.no_grad():
        a, b = model(x, idx=idx), model(x, idx=idx)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="pooling"):
        M.VN_PointNet_CLS(argparse.Namespace(k=k, pooling="sum"))


def test_restatement_equals_the_recorded_stages():
    """The chained restatement on the folded state against every recorded stage, within a tenth of the tests' tolerance."""
    got = dict(PC.restated())
    assert all(v.dtype == F32 for v in got.values()) and got["local"].shape == (2, P.WIDE, 3, 64)
    got["logits"] = P.head_f64(got["h"], PC.state())
    for key in P.STAGES:
        worst = compare_case({"out": got[key]}, {"out": GOLDEN[key]}, 1e-4, "the restatement, %s" % key)
        print("%s: worst relative error %.3e" % (key, worst[0]))


@pytest.mark.parametrize("N,k,O,Od,slope", PC.CROSS_HOST_CASES, ids=lambda v: str(v))
def test_cross_restatement_against_float64_and_the_module(N, k, O, Od, slope):
    seed = 40 + O + Od
    x, idx = synth.normal(seed, 1, (3, N)), synth.integers(seed, 2, (N, k), 3 * N) - N
    a = VC.layer_arrays(seed, 3, O, Od)
    taken = []
    got = P.cross_level(x, idx, P.fold_cross(*(a[key] for key in PC.KEYS)), slope, taken)
    assert got.dtype == F32 and got.shape == (O, 3, N) and len(taken) == 1
    assert 0.1 <= taken[0] <= 0.9, "dot < 0 on %.3f of the pairs: a condition on the inputs" % taken[0]
    compare_case({"out": got}, {"out": P.cross_level_f64(x, idx, a, slope)}, 1e-3, "against the float64 formula")
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross
    layer = VC.layer(None, 3, O, Od == 1, slope, a)
    with torch.no_grad():
        mod = layer(get_graph_feature_cross(torch.from_numpy(x)[None, None], k=k, idx=torch.from_numpy(idx).clamp(0, N - 1)[None])).mean(dim=-1)[0]
    compare_case({"out": got}, {"out": mod.numpy()}, 1e-3, "against the module")


@pytest.mark.parametrize("C,O", PC.NORM_WIDTHS, ids=lambda v: str(v))
def test_norm_only_restatement_against_float64_and_the_modules(C, O):
    N = 17
    x, a = PC.norm_arrays(C, O, N)
    f, want = PC.norm_want(C, O, N)
    assert want.dtype == F32 and want.shape == (2, O, 3, N) and np.isfinite(want).all()
    compare_case({"out": want[0]}, {"out": P.point_norm_f64(x[0], a)}, 1e-3, "against the float64 formula")
    linear, norm = PC.norm_layers(None, C, O, a)
    with torch.no_grad():
        mod = norm(linear(torch.from_numpy(x)))
    compare_case({"out": want}, {"out": mod.numpy()}, 1e-3, "against the modules")


def test_restatement_is_finite_at_the_origin_and_on_duplicated_points():
    x, idx = P.degenerate_cloud()
    assert not x[0, :, 0].any() and np.array_equal(x[0, :, 1], x[0, :, 2])
    a = VC.layer_arrays(5, 3, 21, 21)
    for slope in (0.0, 0.2):
        got = P.cross_level(x[0], idx[0], P.fold_cross(*(a[key] for key in PC.KEYS)), slope)
        assert got.shape == (21, 3, x.shape[2]) and np.isfinite(got).all() and float(np.abs(got).max()) > 0
    e = P.edge_feature(np.ascontiguousarray(x[0].T), np.ascontiguousarray(x[0].T))                # every point against itself
    assert not e[0].any() and not e[2].any()


def test_header_names_the_entries_under_abi_435():
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 435
    names = ("svnet_vn_cross_supported", "svnet_vn_cross_fold_f32", "svnet_vn_edge_cross_mean_f32", "svnet_vn_point_norm_supported",
             "svnet_vn_point_norm_fold_f32", "svnet_vn_point_norm_f32")
    assert "435: " + ", ".join(names) in header and "434: svnet_vn_edge2_supported" in header
    assert "fused vector-neuron cross edge level" in header and "norm-only vector-neuron point layer" in header
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_vn_edge_cross_mean_f32"][1][8] is _lib.c_f
    # every existing entry keeps its argument list
    assert len(_lib.SIGNATURES["svnet_vn_point_supported"][1]) == 5 and len(_lib.SIGNATURES["svnet_vn_point_f32"][1]) == 14
    from svnet_amd import vn_pointnet as VP
    from svnet_amd import vn_tail as VT
    S = VP.supported_cross                                                        # (N, k, O, Od): both sides of every edge
    assert not S(64, 0, 4, 4) and S(64, 1, 4, 4) and S(64, 64, 4, 4) and not S(128, 65, 4, 4)
    assert not S(7, 8, 4, 4) and S(8, 8, 4, 4) and S(32768, 8, 4, 4) and not S(32769, 8, 4, 4)
    assert not S(64, 8, 0, 0) and S(64, 8, 1, 1) and S(64, 8, 128, 128) and not S(64, 8, 129, 129) and not S(64, 8, 129, 1)
    assert S(64, 8, 21, 1) and S(64, 8, 128, 1) and not S(64, 8, 21, 2) and not S(64, 8, 21, 0) and S(1, 1, 21, 21) and S(1024, 20, 21, 21)
    K = VT.supported_point_norm                                                   # (N, C, O)
    assert not K(0, 4, 4) and K(1, 4, 4) and K(32768, 4, 4) and not K(32769, 4, 4)
    assert not K(16, 0, 4) and K(16, 1, 1) and K(16, 512, 512) and not K(16, 513, 4) and not K(16, 4, 0) and not K(16, 4, 513) and K(1024, 42, 341)
    Q = VT.supported_point                                                        # unchanged answers
    assert Q(1, 1, 0, 1, 1) and Q(32768, 512, 512, 512, 1) and not Q(16, 4, 0, 4, 2) and not Q(16, 513, 0, 4, 4)
    L = _lib.lib()
    p = _lib.c_p(64)                                                              # refused before any launch: no device is touched
    E = _lib.DEFINES
    assert L.svnet_vn_edge_cross_mean_f32(None, p, p, 1, 64, 8, 4, 4, 0.0, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge_cross_mean_f32(p, p, p, 0, 64, 8, 4, 4, 0.0, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge_cross_mean_f32(p, p, p, 65536, 64, 8, 4, 4, 0.0, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge_cross_mean_f32(p, p, p, 1, 64, 65, 4, 4, 0.0, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_edge_cross_mean_f32(p, p, p, 1, 4, 8, 4, 4, 0.0, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_edge_cross_mean_f32" in L.svnet_last_error()
    assert L.svnet_vn_cross_fold_f32(p, p, p, p, p, None, 4, 4, 1e-5, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_cross_fold_f32(p, p, p, p, p, p, 129, 129, 1e-5, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_point_norm_f32(p, None, 1, 16, 4, 4, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_point_norm_f32(p, p, 65536, 16, 4, 4, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_point_norm_f32(p, p, 1, 16, 513, 4, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_point_norm_f32" in L.svnet_last_error()
    assert L.svnet_vn_point_norm_fold_f32(p, p, p, p, p, 4, 513, 1e-5, p, None) == E["SVNET_E_UNSUPPORTED"]


_fake = VC.fake


def test_fronts_refuse_bad_arguments_before_any_device_call():
    from svnet_amd import vn_pointnet as VP
    from svnet_amd import vn_tail as VT
    B, N, k, O, C = 2, 16, 4, 5, 3
    x, idx = torch.zeros(B, 1, 3, N), torch.zeros(B, N, k, dtype=torch.int64)
    fx = _fake(VP.FoldedVNCross, O=O, Od=O)
    fn = _fake(VT.FoldedVNPointNorm, C=C, O=O)
    with pytest.raises(TypeError, match="folded must be a FoldedVNCross"):
        VP.vn_edge_cross_mean(x, idx, fn)
    with pytest.raises(TypeError, match="x must be torch.float32"):
        VP.vn_edge_cross_mean(x.double(), idx, fx)
    with pytest.raises(TypeError, match="idx must be torch.int64"):
        VP.vn_edge_cross_mean(x, idx.int(), fx)
    with pytest.raises(ValueError, match="x requires grad"):
        VP.vn_edge_cross_mean(x.clone().requires_grad_(), idx, fx)
    with pytest.raises(ValueError, match=r"x must be \[B,1,3,N\]"):
        VP.vn_edge_cross_mean(torch.zeros(B, 2, 3, N), idx, fx)                   # one vector channel in
    with pytest.raises(ValueError, match=r"x must be \[B,1,3,N\]"):
        VP.vn_edge_cross_mean(torch.zeros(B, 3, N), idx, fx)
    with pytest.raises(ValueError, match=r"idx must be \[B,N,k\]"):
        VP.vn_edge_cross_mean(x, idx[:, :8].contiguous(), fx)
    with pytest.raises(ValueError, match="out must be"):
        VP.vn_edge_cross_mean(x, idx, fx, out=torch.zeros(B, O, N, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # everything in order but the device
        VP.vn_edge_cross_mean(x, idx, fx, out=torch.zeros(B, O, 3, N))
    xp = torch.zeros(B, C, 3, N)
    with pytest.raises(TypeError, match="folded must be a FoldedVNPointNorm"):
        VT.vn_point_norm(xp, fx)
    with pytest.raises(TypeError, match="folded must be a FoldedVNPoint "):
        VT.vn_point(xp, fn)
    with pytest.raises(TypeError, match="x must be torch.float32"):
        VT.vn_point_norm(xp.double(), fn)
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VT.vn_point_norm(torch.zeros(B, C, N), fn)
    with pytest.raises(ValueError, match="the layer takes 3 vector channels"):
        VT.vn_point_norm(torch.zeros(B, C + 1, 3, N), fn)
    with pytest.raises(ValueError, match="out must be"):
        VT.vn_point_norm(xp, fn, out=torch.zeros(B, C, 3, N))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.vn_point_norm(xp, fn, out=torch.zeros(B, O, 3, N))
    # the folds: the wrong layers, the wrong width, and layers that are not on a HIP device
    from svnet_amd.models.vn_layers import VNBatchNorm, VNLinear, VNLinearLeakyReLU
    with pytest.raises(TypeError, match="needs a VNLinearLeakyReLU"):
        VP.fold_vn_cross(VNLinear(3, O))
    with pytest.raises(ValueError, match="has 3"):
        VP.fold_vn_cross(VNLinearLeakyReLU(4, O))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VP.fold_vn_cross(VNLinearLeakyReLU(3, O))
    with pytest.raises(TypeError, match="needs a VNLinear and a VNBatchNorm"):
        VT.fold_vn_linear_norm(VNLinearLeakyReLU(3, O), VNBatchNorm(O, dim=4))
    with pytest.raises(ValueError, match="the widths differ"):
        VT.fold_vn_linear_norm(VNLinear(3, O), VNBatchNorm(O + 1, dim=4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VT.fold_vn_linear_norm(VNLinear(3, O), VNBatchNorm(O, dim=4))


def test_wrapper_refuses_what_it_cannot_take():
    from svnet_amd import vn_pointnet as VP
    with pytest.raises(TypeError, match="VN_PointNet_CLS"):
        VP.FusedVNPointNet(VC.golden_model())                                     # (the DGCNN classifier)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VP.FusedVNPointNet(PC.golden_model())
    # pooling = 'max' and normalize_frame: nothing to fold, so the wrapper lives on the CPU too; every call is the model's
    framed = PC.golden_model()
    framed.feat.std_feature.normalize_frame = True
    x, idx = torch.from_numpy(GOLDEN["x"]), torch.from_numpy(GOLDEN["idx"])
    for model in (PC.golden_model(pooling="max"), framed):
        fused = VP.FusedVNPointNet(model)
        assert not fused.fused and fused.cross is None and not fused.points and not fused.supported(2, 64, 8)
        VC.cpu_wrapper_refuses(fused, (x,), [
            (TypeError, "x must be torch.float32", (x.double(),), {}),
            (ValueError, "x requires grad", (x.clone().requires_grad_(),), {}),
            (ValueError, r"x must be \[B,3,N\]", (x[:, :2].contiguous(),), {}),
            (ValueError, "neighbour list", (x,), {"idx": [idx]}),
            (RuntimeError, "no CPU fallback", (x,), {"idx": idx})])
