"""CPU tests of the vector-neuron baseline: the modules of svnet_amd/models/vn_layers.py, models/utils/vn_util.py and
models/vn_dgcnn_cls.py and the numpy restatement tests/vn_ref.py against the reference's recorded run (tests/golden/vn.npz, neighbour
lists replayed), the header's new entry points, and the refusals of svnet_amd/vn_fused.py that need no device.  The kernels
themselves: tests/test_hip_vn.py."""
import functools
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib
from tests import vn_cases as VC
from tests import vn_ref as V
from tests.common import compare_case

F32 = np.float32
GOLDEN = VC.GOLDEN
golden_state, golden_model = VC.state, functools.partial(VC.golden_model, None)


def golden_lists():
    return [torch.from_numpy(GOLDEN["idx%d" % i]) for i in range(4)]


def test_state_dict_layout_equals_the_recorded_one_and_loads_strictly():
    seed, B, N, k, num_class = V.GOLDEN_CASE
    model = golden_model()                                                       # (the strict load is inside)
    mine = model.state_dict()
    assert list(mine) == [str(key) for key in GOLDEN["keys"]]
    for key, shape in zip(GOLDEN["keys"], GOLDEN["shapes"]):
        assert tuple(mine[str(key)].shape) == tuple(int(v) for v in shape if v >= 0), key
    state = golden_state()
    for key in mine:
        if key.endswith("bn.weight"):
            assert (state[key] > 0).any() and (state[key] < 0).any(), key
        if key.endswith("running_var"):
            assert (np.abs(state[key] - 1) > 0.05).any()
    assert GOLDEN["x"].shape == (B, 3, N) and np.array_equal(GOLDEN["x"], V.golden_cloud()) and GOLDEN["logits"].shape == (B, num_class)
    assert all(GOLDEN["idx%d" % i].shape == (B, N, k) and GOLDEN["lvl%d" % i].shape == (B, V.LEVEL_WIDTHS[i][1], 3, N) for i in range(4))


def test_modules_equal_the_recorded_levels_and_logits():
    """The reference's lists replayed into the module on the CPU: every level's output and the logits within the project's 1e-3."""
    model = golden_model()
    levels = []
    hooks = [conv.register_forward_hook(lambda mod, inp, out: levels.append(out.mean(dim=-1))) for conv, _ in model.edge_levels()]
    with torch.no_grad():
        logits = model(torch.from_numpy(GOLDEN["x"]), idx=golden_lists())
    for h in hooks:
        h.remove()
    got = {"out:lvl%d" % i: levels[i].numpy() for i in range(4)}
    got["out:logits"] = logits.numpy()
    ref = {"out:lvl%d" % i: GOLDEN["lvl%d" % i] for i in range(4)}
    ref["out:logits"] = GOLDEN["logits"]
    worst = compare_case(got, ref, 1e-3, "vn.npz")
    print("worst relative error %.3e at %s" % worst)
    with pytest.raises(ValueError, match="four levels"):
        model(torch.from_numpy(GOLDEN["x"]), idx=golden_lists()[:3])


def test_restatement_equals_the_recorded_levels_and_logits():
    """tests/vn_ref.py on the folded state: each level on its recorded input, then the four levels chained and the model's own tail."""
    seed, B, N, k, num_class = V.GOLDEN_CASE
    state = golden_state()
    x = GOLDEN["x"][:, None]
    h, got = x, {}
    for i, prefix in enumerate(V.LEVEL_PREFIXES):
        f = V.fold_state(state, prefix)
        recorded_in = x if i == 0 else GOLDEN["lvl%d" % (i - 1)]
        taken = []
        got["out:lvl%d" % i] = np.stack([V.level(recorded_in[b], GOLDEN["idx%d" % i][b], f, V.SLOPE, taken) for b in range(B)])
        assert 0.1 <= np.mean(taken) <= 0.9, (i, taken)                          # both branches of the leaky rule are exercised
        h = V.level_batch(h, GOLDEN["idx%d" % i], f)
        got["out:chained%d" % i] = h
    ref = {"out:lvl%d" % i: GOLDEN["lvl%d" % i] for i in range(4)}
    ref.update({"out:chained%d" % i: GOLDEN["lvl%d" % i] for i in range(4)})
    with torch.no_grad():
        feats = [torch.from_numpy(got["out:chained%d" % i]) for i in range(4)]
        got["out:logits"] = golden_model().tail(feats).numpy()
    ref["out:logits"] = GOLDEN["logits"]
    worst = compare_case(got, ref, 1e-3, "the restatement")
    print("worst relative error %.3e at %s" % worst)


@pytest.mark.parametrize("C,O,Od,N,k,slope", [(1, 21, 21, 20, 5, 0.2), (5, 7, 1, 9, 9, 0.0), (3, 4, 4, 6, 2, 0.2)])
def test_restatement_lies_at_fp32_noise_from_the_float64_definition(C, O, Od, N, k, slope):
    from svnet_amd import synth
    x = synth.normal(60 + C, 1, (C, 3, N))
    idx = synth.integers(60 + C, 2, (N, k), N)
    a = VC.layer_arrays(60 + C, 2 * C, O, Od)
    got = V.level(x, idx, V.fold(**a), slope)
    want = V.level_f64(x, idx, **a, slope=slope)
    assert got.dtype == F32 and got.shape == want.shape == (O, 3, N)
    # a few dozen fp32 roundings per value, some of them amplified by the division by the norm: 2e-5 of the largest output is two
    # hundred ulps of room, a fiftieth of the project's 1e-3
    assert float(np.abs(got - want).max()) <= 2e-5 * float(np.abs(want).max())


def test_graph_features_equal_the_recorded_tensors_exactly():
    from svnet_amd.models.utils import vn_util as U
    x, idx = V.graph_inputs()
    assert np.array_equal(x, GOLDEN["gf_x"]) and np.array_equal(idx, GOLDEN["gf_idx"])
    tx, tidx = torch.from_numpy(x), torch.from_numpy(idx)
    seed, B, C, N, k = V.GRAPH_CASE
    got = U.get_graph_feature(tx, k=k, idx=tidx)
    assert tuple(got.shape) == (B, 2 * C, 3, N, k) and got.is_contiguous() and np.array_equal(got.numpy(), GOLDEN["gf_out"])
    got = U.get_graph_feature_cross(tx, k=k, idx=tidx)
    assert tuple(got.shape) == (B, 3 * C, 3, N, k) and got.is_contiguous() and np.array_equal(got.numpy(), GOLDEN["gfc_out"])
    assert GOLDEN["gfc_out"][:, 2 * C:].any()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # the dynamic graph is the library's kernel
        U.get_graph_feature(tx, k=k)


def test_layers_keep_the_reference_definitions():
    """share_nonlinearity gives one direction row; VNBatchNorm is x / (|x| + EPS) * bn(|x| + EPS); VNMaxPool picks whole vectors."""
    from svnet_amd.models import vn_layers as L
    assert L.EPS == 1e-6
    assert tuple(L.VNLinearLeakyReLU(4, 6, share_nonlinearity=True).map_to_dir.weight.shape) == (1, 4)
    assert tuple(L.VNLeakyReLU(4, share_nonlinearity=True).map_to_dir.weight.shape) == (1, 4)
    torch.manual_seed(3)
    x = torch.randn(2, 4, 3, 5, 6)
    bn = L.VNBatchNorm(4, dim=5).eval()
    with torch.no_grad():
        bn.bn.running_mean.uniform_(-0.5, 0.5)
        bn.bn.weight.uniform_(-1, 1)
        norm = torch.sqrt((x * x).sum(2)) + L.EPS
        want = x / norm.unsqueeze(2) * bn.bn(norm).unsqueeze(2)
        assert torch.allclose(bn(x), want, rtol=1e-6, atol=1e-7)
        pool = L.VNMaxPool(4)
        got = pool(x)
        d = pool.map_to_dir(x.transpose(1, -1)).transpose(1, -1)
        best = (x * d).sum(2).argmax(-1)                                          # [B,C,N]
        for b, c, n in [(0, 0, 0), (1, 3, 4), (0, 2, 1)]:
            assert torch.equal(got[b, c, :, n], x[b, c, :, n, best[b, c, n]])
        assert tuple(got.shape) == (2, 4, 3, 5) and torch.equal(L.mean_pool(x), x.mean(-1))
        # the leaky rule is continuous across dot = 0 and leaves vectors along their direction alone
        act = L.VNLeakyReLU(4, negative_slope=0.0)
        y = act(x)
        dd = act.map_to_dir(x.transpose(1, -1)).transpose(1, -1)
        # nothing points against its direction afterwards: what is left of a negative projection is dot EPS / (|d|^2 + EPS), and a
        # few fp32 roundings of the products' magnitudes
        dot, scale = (x * dd).sum(2), (x.abs() * dd.abs()).sum(2)
        assert bool(((y * dd).sum(2) >= -(dot.abs() * L.EPS / ((dd * dd).sum(2) + L.EPS)) - 4e-6 * scale).all()) and bool((dot < 0).any())
        xs, z = L.VNStdFeature(8, dim=4)(torch.randn(2, 8, 3, 5))
        assert tuple(xs.shape) == (2, 8, 3, 5) and tuple(z.shape) == (2, 3, 3, 5)


def test_header_names_the_new_entry_points_under_the_bumped_abi():
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 432
    assert "432: svnet_vn_fold_f32, svnet_vn_tables_f32, svnet_vn_edge_mean_f32, svnet_vn_supported, svnet_vn_workspace_bytes" in header
    assert "fused vector-neuron edge level" in header
    for name in ("svnet_vn_fold_f32", "svnet_vn_tables_f32", "svnet_vn_edge_mean_f32", "svnet_vn_supported", "svnet_vn_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["svnet_vn_workspace_bytes"][0] is _lib.c_sz and _lib.SIGNATURES["svnet_vn_edge_mean_f32"][1][10] is _lib.c_f
    from svnet_amd import vn_fused as VF
    # both sides of every edge of the envelope: k 0 / 1 / 64 / 65, N k-1 / k / 32768 / 32769, C and O 0 / 1 / 128 / 129, Od O / 1 / other
    assert not VF.supported(16, 0, 4, 4, 4) and VF.supported(16, 1, 4, 4, 4) and VF.supported(64, 64, 4, 4, 4) and not VF.supported(65, 65, 4, 4, 4)
    assert not VF.supported(7, 8, 4, 4, 4) and VF.supported(8, 8, 4, 4, 4) and VF.supported(32768, 8, 4, 4, 4) and not VF.supported(32769, 8, 4, 4, 4)
    assert not VF.supported(16, 8, 0, 4, 4) and VF.supported(16, 8, 1, 4, 4) and VF.supported(16, 8, 128, 4, 4) and not VF.supported(16, 8, 129, 4, 4)
    assert not VF.supported(16, 8, 4, 0, 0) and VF.supported(16, 8, 4, 1, 1) and VF.supported(16, 8, 4, 128, 128) and not VF.supported(16, 8, 4, 129, 129)
    assert VF.supported(16, 8, 4, 7, 1) and not VF.supported(16, 8, 4, 7, 2) and not VF.supported(16, 8, 4, 7, 0)
    assert all(VF.supported(1024, 20, C, O, O) for C, O in V.LEVEL_WIDTHS)
    L = _lib.lib()
    assert L.svnet_vn_workspace_bytes(32, 1024, 85, 85) == 2 * 32 * 1024 * 3 * 170 * 4 and L.svnet_vn_workspace_bytes(2, 9, 7, 1) == 2 * 2 * 9 * 3 * 8 * 4
    assert L.svnet_vn_workspace_bytes(1, 16, 129, 129) == 0 and L.svnet_vn_workspace_bytes(0, 16, 4, 4) == 0
    p = _lib.c_p(64)                                                              # refused before any launch: no device is touched
    E = _lib.DEFINES
    assert L.svnet_vn_fold_f32(None, p, p, p, p, p, 4, 4, 4, 1e-5, p, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_fold_f32(p, p, p, p, p, p, 4, 4, 2, 1e-5, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert L.svnet_vn_tables_f32(p, p, 1, 16, 4, 4, 4, None, 0, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_tables_f32(p, p, 1, 16, 4, 4, 4, p, 16, None) == E["SVNET_E_WORKSPACE"]
    assert L.svnet_vn_tables_f32(p, p, 65536, 16, 4, 4, 4, p, 1 << 40, None) == E["SVNET_E_ARG"]
    assert L.svnet_vn_edge_mean_f32(p, 1 << 20, p, p, 1, 16, 17, 4, 4, 4, 0.2, p, None) == E["SVNET_E_UNSUPPORTED"]
    assert b"svnet_vn_edge_mean_f32" in L.svnet_last_error()
    assert L.svnet_vn_edge_mean_f32(p, 16, p, p, 1, 16, 8, 4, 4, 4, 0.2, p, None) == E["SVNET_E_WORKSPACE"]
    assert L.svnet_vn_edge_mean_f32(p, 1 << 20, None, p, 1, 16, 8, 4, 4, 4, 0.2, p, None) == E["SVNET_E_ARG"]


def _fake_folded(C, O, Od=None):
    from svnet_amd import vn_fused as VF
    return VC.fake(VF.FoldedVNLayer, C=C, O=O, Od=O if Od is None else Od)


def test_vn_edge_mean_refuses_bad_arguments():
    from svnet_amd import vn_fused as VF
    B, C, N, k, O = 2, 3, 16, 4, 5
    x, idx, f = torch.zeros(B, C, 3, N), torch.zeros(B, N, k, dtype=torch.int64), _fake_folded(C, O)
    with pytest.raises(TypeError, match="FoldedVNLayer"):
        VF.vn_edge_mean(x, idx, object())
    with pytest.raises(TypeError, match="x must be torch.float32"):
        VF.vn_edge_mean(x.double(), idx, f)
    with pytest.raises(TypeError, match="idx must be torch.int64"):
        VF.vn_edge_mean(x, idx.int(), f)
    with pytest.raises(TypeError, match="idx must be a tensor"):
        VF.vn_edge_mean(x, idx.numpy(), f)
    with pytest.raises(ValueError, match="x requires grad"):
        VF.vn_edge_mean(x.clone().requires_grad_(), idx, f)
    with pytest.raises(ValueError, match="x must be contiguous"):
        VF.vn_edge_mean(torch.zeros(B, C, N, 3).transpose(2, 3), idx, f)
    with pytest.raises(ValueError, match=r"x must be \[B,C,3,N\]"):
        VF.vn_edge_mean(torch.zeros(B, C, N), idx, f)
    with pytest.raises(ValueError, match=r"idx must be \[B,N,k\]"):
        VF.vn_edge_mean(x, torch.zeros(B, N - 1, k, dtype=torch.int64), f)
    with pytest.raises(ValueError, match="the layer takes 4 vector channels"):
        VF.vn_edge_mean(x, idx, _fake_folded(4, O))
    with pytest.raises(ValueError, match="out must be"):
        VF.vn_edge_mean(x, idx, f, out=torch.zeros(B, O, N, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # everything in order but the device
        VF.vn_edge_mean(x, idx, f, out=torch.zeros(B, O, 3, N))


def test_fold_and_wrapper_refuse_what_they_cannot_take():
    from svnet_amd import vn_fused as VF
    from svnet_amd.models import vn_layers as L
    with pytest.raises(TypeError, match="VNLinearLeakyReLU"):
        VF.fold_vn_layer(L.VNLinear(4, 4))
    with pytest.raises(TypeError, match="VNLinearLeakyReLU"):
        VF.fold_vn_layer(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="even input width"):
        VF.fold_vn_layer(L.VNLinearLeakyReLU(5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.fold_vn_layer(L.VNLinearLeakyReLU(4, 4))
    with pytest.raises(TypeError, match="VN_DGCNN_CLS"):
        VF.FusedVNDGCNN(torch.nn.Linear(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.FusedVNDGCNN(golden_model())
    fused = VF.FusedVNDGCNN(golden_model("max"))                                 # nothing to fold: every call is the model's
    assert not fused.supported(64, 8) and isinstance(fused, torch.nn.Module) and fused.model.pool1.map_to_dir.weight.shape == (21, 21)
    x, flat = torch.zeros(2, 3, 64), torch.zeros(2, 64, 3)
    VC.cpu_wrapper_refuses(fused, (x,), [
        (TypeError, "x must be torch.float32", (x.double(),), {}),
        (ValueError, r"x must be \[B,3,N\]", (flat,), {}),
        (ValueError, "x requires grad", (flat.transpose(1, 2).requires_grad_(),), {}),      # asked of the argument, a view included
        (ValueError, "x requires grad", (x.clone().requires_grad_(),), {}),
        (ValueError, "four levels", (x,), {"idx": golden_lists()[:2]}),
        (ValueError, r"idx\[1\] on meta", (x,), {"idx": [i.to("meta") if n == 1 else i for n, i in enumerate(golden_lists())]}),      # every list on x's device
        (RuntimeError, "no CPU fallback", (x,), {"idx": golden_lists()})], mode=fused)
    assert fused.release() is fused
    f = _fake_folded(3, 5)
    f._ws = VF._vn.Workspace(f.device)
    f._ws._retired = [torch.zeros(4)]
    assert f.release() is f and f._ws._retired == []
    with pytest.raises(ValueError, match="pooling must be"):
        golden_model("median")
    with pytest.raises(ValueError, match="dim must be 3, 4 or 5"):
        L.VNBatchNorm(4, dim=2)
