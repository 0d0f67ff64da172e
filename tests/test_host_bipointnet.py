"""BiPointNet_CLS on the CPU: the modules against the reference's recorded run (tests/golden/bipointnet.npz), the numpy restatement of
the fused chain's contract (tests/bi_ref.py) against the same, and the host side of svnet_amd/bi_fused.py - the `supported`
predicates at each limit and one past it, every argument check of bi_chain, the wrapper's refusals, the ABI."""
import os
import re
import types

import numpy as np
import pytest
import torch

import svnet_amd.models as M
from svnet_amd import _lib, bi_fused as F
from svnet_amd.models import bipointnet as BP
from svnet_amd.models.bipointnet_basic import BiLinearLSR, BinaryQuantize
from tests import bi_ref as R
from tests.common import compare_case, load_npz

GRADS = ["fc3.weight", "feat.conv1.lin.weight", "feat.stn.fc3.weight"]


@pytest.fixture(scope="module")
def golden():
    g = load_npz("bipointnet.npz")
    seed, B, N, num_class = R.GOLDEN_CASE
    state = R.synthetic_state(g["keys"], g["shapes"], seed)
    return g, state


def _model(state):
    model = M.BiPointNet_CLS(types.SimpleNamespace(), R.GOLDEN_CASE[3])
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    return model


def test_state_dict_layout_is_the_recorded_one(golden):
    g, state = golden
    layout = M.BiPointNet_CLS(types.SimpleNamespace(), R.GOLDEN_CASE[3]).state_dict()
    assert list(layout) == [str(k) for k in g["keys"]]
    assert [list(v.shape) + [-1] * (2 - v.dim()) for v in layout.values()] == g["shapes"].tolist()
    assert M.BiPointNet_CLS is BP.BiPointNetLSREMax and "BiPointNet_CLS" in M.__all__
    assert BP.offset_map == R.OFFSET_MAP
    for key, v in state.items():
        if key.endswith(".scale"):
            assert 0.02 <= float(v) <= 0.08
        if key.endswith("running_var"):
            assert 0.5 <= v.min() and v.max() <= 1.5
        if key.endswith("running_mean"):
            w = state[key[:-len("running_mean")] + "weight"]
            assert (w > 0).any() and (w < 0).any()


def test_eval_outputs_equal_the_recorded_ones(golden):
    g, state = golden
    model = _model(state).eval()
    seen = {}
    hooks = [model.feat.stn.register_forward_hook(lambda m, i, o: seen.__setitem__("trans", o)),
             model.feat.stn.fc1.register_forward_pre_hook(lambda m, i: seen.__setitem__("pool_stn", i[0])),
             model.feat.fstn.fc1.register_forward_pre_hook(lambda m, i: seen.__setitem__("pool_fstn", i[0])),
             model.fc1.register_forward_pre_hook(lambda m, i: seen.__setitem__("pool", i[0]))]
    with torch.no_grad():
        seen["logits"], seen["trans_feat"] = model(torch.from_numpy(g["x"]))
    for h in hooks:
        h.remove()
    for key in R.STAGES:
        assert np.array_equal(seen[key].numpy(), g[key]), key          # the same operations on the same build


def test_train_pass_matches_the_recorded_logits_and_gradients(golden):
    g, state = golden
    model = _model(state).train()
    logits, _ = model(torch.from_numpy(g["x"]))
    logits.sum().backward()
    params = dict(model.named_parameters())
    got = {"train:logits": logits.detach().numpy()}
    got.update({"d:" + k: params[k].grad.numpy() for k in GRADS})
    compare_case(got, {k: g[k] for k in got}, 1e-6, "train")


def test_binary_quantize_is_sign_with_a_clipped_straight_through_gradient():
    x = torch.tensor([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], requires_grad=True)
    y = BinaryQuantize.apply(x)
    assert y.tolist() == [-1, -1, -1, 0, 1, 1, 1]
    y.backward(torch.full((7,), 3.0))
    assert x.grad.tolist() == [0, 3, 3, 3, 3, 3, 0]


def test_first_call_sets_every_scale_and_the_all_zero_corner():
    torch.manual_seed(0)
    model = M.BiPointNet_CLS(types.SimpleNamespace(), 40).train()
    layers = [m for m in model.modules() if isinstance(m, BiLinearLSR)]
    assert len(layers) == len(R.BI_LAYERS) and all(float(m.scale.detach()) == 0.0 and m.scale.dim() == 0 and m.bias is None for m in layers)
    model(torch.randn(2, 3, 1024))
    assert all(float(m.scale.detach()) > 0.0 and m.scale.dim() == 0 for m in layers)
    assert set(k for k, m in model.named_modules() if isinstance(m, BiLinearLSR)) == set(R.BI_LAYERS)
    lin = BiLinearLSR(16, 8)
    out = lin(torch.zeros(4, 16))                                       # 0 / 0 -> the weights' own ratio
    bw = lin.weight - lin.weight.mean()
    assert float(lin.scale.detach()) == float(bw.std() / torch.sign(bw).std()) and not out.any()
    assert BiLinearLSR(4, 4, bias=True).bias is not None and not BiLinearLSR(4, 4, binary_act=False).binary_act


def test_a_cloud_size_without_an_offset_raises_key_error():
    model = M.BiPointNet_CLS(types.SimpleNamespace(), 40).eval()
    with pytest.raises(KeyError):
        model(torch.randn(2, 3, 512))


def test_restatement_against_the_golden(golden):
    g, state = golden
    got, signs = R.forward(g["x"], state)
    for key in R.BI_LAYERS:
        assert np.array_equal(signs[key], R.unpack_signs(g["sp:" + key], g["sz:" + key], signs[key].shape[1])), key
        assert (signs[key] > 0).mean() >= 0.1 and (signs[key] < 0).mean() >= 0.1
    compare_case({"out:" + k: got[k] for k in R.STAGES}, {"out:" + k: g[k] for k in R.STAGES}, 1e-4, "restatement")
    for key in R.BI_LAYERS:                                             # the fold's signs are the module's expression
        w = torch.from_numpy(state[key + ".weight"])
        assert np.array_equal(R.fold_state_bi(state, key)["S"], torch.sign(w - w.mean()).numpy().astype(np.int8)), key


def test_restatement_primitives():
    rng = np.random.default_rng(0)
    W = rng.standard_normal((7, 300)).astype(np.float32)
    assert abs(R.weight_sum(W) - float(np.sum(W.astype(np.float64)))) < 1e-9
    f = R.fold_bi(np.full((3, 4), 0.125, dtype=np.float32), 0.05)
    assert not f["S"].any() and np.array_equal(f["a"], np.full(3, np.float32(0.05))) and not f["b"].any()
    x = rng.standard_normal((1, 4, 9)).astype(np.float32)
    same = R.chain(x, [("bi", R.fold_bi(rng.standard_normal((5, 4)).astype(np.float32), 0.5))], clamp=False)
    eye = R.chain(x, [("bi", R.fold_bi(rng.standard_normal((5, 4)).astype(np.float32), 0.5))], trans=np.eye(4, dtype=np.float32)[None], clamp=False)
    assert same.shape == eye.shape == (1, 5, 9)
    s = R.sgn(rng.standard_normal((6, 13)))
    s[0, :3] = 0
    assert np.array_equal(R.unpack_signs(*R.pack_signs(s), 13), s)


def test_supported_at_each_limit_and_one_past_it():
    ok = F.supported
    assert F.rows_tile() == 128
    assert ok(3, 1, [64]) and ok(3, 32768, [64]) and not ok(3, 0, [64]) and not ok(3, 32769, [64])
    assert ok(3, 8, [8, 8, 8, 8]) and not ok(3, 8, [8] * 5) and not ok(3, 8, [])
    assert ok(64, 8, [8], trans=True) and not ok(65, 8, [8], trans=True) and ok(65, 8, [8])
    assert ok(64, 8, [512], first_fp=True) and not ok(65, 8, [8], first_fp=True) and not ok(64, 8, [513], first_fp=True)
    assert ok(512, 8, [8]) and not ok(513, 8, [8])
    assert ok(8, 8, [512, 8]) and not ok(8, 8, [513, 8])
    assert ok(8, 8, [2048]) and not ok(8, 8, [2049]) and ok(8, 8, [512, 2048]) and not ok(8, 8, [0])
    assert ok(128, 2048, [512, 2048])                                  # the part-segmentation model's widest layers
    L = _lib.lib()
    assert L.svnet_bi_chain_workspace_bytes(2, 128, 1024) == 0 and L.svnet_bi_chain_workspace_bytes(2, 129, 1024) == 2 * 2 * 1024 * 4
    assert L.svnet_bi_chain_workspace_bytes(65536, 129, 8) == 0
    assert L.svnet_bi_packed_bytes(1024, 128) == 1024 * 128 and L.svnet_bi_packed_bytes(9, 3) == 32 * 32 and L.svnet_bi_packed_bytes(8, 513) == 0


def _fake(cls, K, O, device="cpu"):
    """A stand-in for a folded layer: the real class with placeholder fields (bi_chain checks types first)."""
    f = cls.__new__(cls)
    f.K, f.O, f.device = K, O, torch.device(device)
    f.w_i8 = torch.zeros(1, dtype=torch.int8) if K <= 512 else None
    f.w = f.ab = torch.zeros(1)
    return f


def test_every_argument_check_of_bi_chain():
    x = torch.zeros(2, 3, 16)
    fp, bi = _fake(F.FoldedFp, 3, 8), _fake(F.FoldedBi, 8, 4)
    with pytest.raises(ValueError, match="1 .. 4 folded layers"):
        F.bi_chain(x, [])
    with pytest.raises(ValueError, match="1 .. 4 folded layers"):
        F.bi_chain(x, [fp] + [bi] * 4)
    with pytest.raises(TypeError, match=r"layers\[0\] must be a FoldedBi .* or a FoldedFp"):
        F.bi_chain(x, [object()])
    with pytest.raises(TypeError, match=r"layers\[1\] must be a FoldedBi"):
        F.bi_chain(x, [fp, fp])
    with pytest.raises(ValueError, match="pool must be None or 'max'"):
        F.bi_chain(x, [fp], pool="mean")
    with pytest.raises(TypeError, match="x must be a tensor"):
        F.bi_chain(None, [fp])
    with pytest.raises(TypeError, match="x must be torch.float32"):
        F.bi_chain(x.double(), [fp])
    with pytest.raises(ValueError, match="x must be contiguous"):
        F.bi_chain(x.transpose(1, 2), [fp])
    for key in ("x", "trans", "out"):
        args = {"x": x.clone(), "trans": torch.zeros(2, 3, 3), "out": torch.zeros(2, 8, 16)}
        args[key].requires_grad_(True)
        with pytest.raises(ValueError, match="%s requires grad" % key):
            F.bi_chain(args["x"], [fp], trans=args["trans"], out=args["out"])
    with pytest.raises(ValueError, match=r"x must be \[B,C0,N\]"):
        F.bi_chain(torch.zeros(3, 16), [fp])
    with pytest.raises(ValueError, match=r"trans must be \[B,C0,C0\]"):
        F.bi_chain(x, [fp], trans=torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match=r"layers\[0\] takes 3 channels, x has 5"):
        F.bi_chain(torch.zeros(2, 5, 16), [fp])
    with pytest.raises(ValueError, match=r"layers\[2\] takes 8 channels, the layer before has 4"):
        F.bi_chain(x, [fp, bi, bi])
    with pytest.raises(_lib.SvnetHipError, match="at most 512"):
        F.bi_chain(torch.zeros(2, 1024, 16), [_fake(F.FoldedBi, 1024, 8)])
    with pytest.raises(ValueError, match=r"out must be \[B,O,N\]"):
        F.bi_chain(x, [fp], out=torch.zeros(2, 8, 15))
    with pytest.raises(ValueError, match=r"out must be \[B,O\]"):
        F.bi_chain(x, [fp], pool="max", out=torch.zeros(2, 8, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.bi_chain(x, [fp, bi])


def test_fold_refusals():
    with pytest.raises(TypeError, match="needs a BiLinearLSR"):
        F.fold_bi_layer(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="reset_scale"):
        F.fold_bi_layer(BiLinearLSR(4, 4))
    lin = BiLinearLSR(4, 4)
    lin.scale.data.fill_(0.05)
    with pytest.raises(ValueError, match="binary_act"):
        F.fold_bi_layer(BiLinearLSR(4, 4, binary_act=False))
    with pytest.raises(TypeError, match="BatchNorm1d"):
        F.fold_bi_layer(lin, torch.nn.LayerNorm(4))
    with pytest.raises(ValueError, match="affine"):
        F.fold_bi_layer(lin, torch.nn.BatchNorm1d(4, affine=False))
    with pytest.raises(ValueError, match="BatchNorm over 5"):
        F.fold_bi_layer(lin, torch.nn.BatchNorm1d(5))
    with pytest.raises(RuntimeError, match="needs a HIP"):
        F.fold_bi_layer(lin, torch.nn.BatchNorm1d(4))
    with pytest.raises(TypeError, match="full-precision"):
        F.fold_fp_layer(lin, torch.nn.BatchNorm1d(4))
    with pytest.raises(ValueError, match="must have a bias"):
        F.fold_fp_layer(torch.nn.Linear(4, 4, bias=False), torch.nn.BatchNorm1d(4))
    with pytest.raises(RuntimeError, match="needs a HIP"):
        F.fold_fp_layer(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))


def test_wrapper_refusals_and_fallback_conditions():
    with pytest.raises(TypeError, match="needs a BasicBiPointNet"):
        F.FusedBiPointNet(torch.nn.Linear(3, 3))
    fresh = M.BiPointNet_CLS(types.SimpleNamespace(), 40).eval()
    fused = F.FusedBiPointNet(fresh)                                    # scales still 0: nothing is folded, no device is needed
    assert not fused.fused and not fused.supported(2, 1024) and not fused.training
    fresh.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(torch.zeros(2, 3, 1024))
    fresh.eval()
    with pytest.raises(ValueError, match="requires grad"):
        fused(torch.zeros(2, 3, 1024, requires_grad=True))
    with pytest.raises(ValueError, match=r"x must be \[B,3,N\]"):
        fused(torch.zeros(2, 4, 1024))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused(torch.zeros(2, 3, 1024))
    for kw in ({"bi_last": True}, {"bi_first": True}, {"pool": "max"}, {"tnet": False}, {"use_bn": False}, {"affine": False}):
        args = dict(k=40, Linear=BiLinearLSR, pool="ema-max")
        args.update(kw)
        other = BP.BasicBiPointNet(**args).eval()
        for m in other.modules():
            if isinstance(m, BiLinearLSR):
                m.scale.data.fill_(0.05)
        assert not F.FusedBiPointNet._fusable(other), kw
    model = M.BiPointNet_CLS(types.SimpleNamespace(), 40).eval()
    for m in model.modules():
        if isinstance(m, BiLinearLSR):
            m.scale.data.fill_(0.05)
    assert F.FusedBiPointNet._fusable(model)
    with pytest.raises(RuntimeError, match="needs a HIP"):
        F.FusedBiPointNet(model)


def test_header_names_the_new_entries_under_abi_438():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svnet_hip.h")).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 438
    names = ["svnet_bi_packed_bytes", "svnet_bi_fold_f32", "svnet_bi_chain_supported", "svnet_bi_chain_rows_tile",
             "svnet_bi_chain_workspace_bytes", "svnet_bi_chain_f32"]
    assert "438: " + ", ".join(names) in header
    assert all(n in _lib.SIGNATURES and hasattr(_lib.lib(), n) for n in names)
