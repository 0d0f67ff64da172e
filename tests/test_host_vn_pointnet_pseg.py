"""CPU tests of the vector-neuron PointNet for part segmentation: the torch model svnet_amd.models.VN_PointNet_PSEG against the
reference's recorded run (tests/golden/vn_pointnet_pseg.npz), the chained numpy restatement tests/vn_pointnet_pseg_ref.py against the
same recordings, the wide envelope of the vector tail as the header and the host functions state it, and the refusals of
vn_pointnet_pseg.FusedVNPointNetPSeg that need no device.  The kernels themselves: tests/test_hip_vn_pointnet_pseg.py."""
import argparse
import re

import numpy as np
import pytest
import torch

from svnet_amd import _lib, synth
from tests import vn_cases as VC
from tests import vn_pointnet_pseg_cases as PC
from tests import vn_pointnet_pseg_ref as P
from tests.common import compare_case

F32 = np.float32
GOLDEN = PC.GOLDEN

WIDE_NAMES = ("svnet_vn_point_wide_supported", "svnet_vn_point_wide_workspace_bytes", "svnet_vn_point_wide_fold_f32", "svnet_vn_point_wide_f32",
              "svnet_vn_point_norm_wide_supported", "svnet_vn_point_norm_wide_fold_f32", "svnet_vn_point_norm_wide_f32", "svnet_vn_cloud_mean_wide_f32",
              "svnet_vn_std_pool_wide_supported", "svnet_vn_std_pool_wide_workspace_bytes", "svnet_vn_std_pool_wide_f32",
              "svnet_vn_std_coords_wide_supported", "svnet_vn_std_coords_wide_f32")


def _model_stages(model, x, l, idx):
    """{stage: array} of the module's forward on the list idx, by the model's own accessors."""
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross
    B, _, N = x.shape
    with torch.no_grad():
        logits = model(x, l, idx=idx)
        conv_pos, pool = model.position_level()
        pos = pool(conv_pos(get_graph_feature_cross(x.unsqueeze(1), k=model.k, idx=idx)))
        out1, out2, out3, g, out4 = model.point_features(pos)
        out5, frame = model.invariant(out4)
        h = out5.max(dim=-1)[0]
        e1234 = torch.einsum('bijm,bjkm->bikm', torch.cat((out1, out2, out3, out4), dim=1), frame).reshape(B, -1, N)
        concat = torch.cat((torch.cat((h, l), dim=1).unsqueeze(-1).expand(-1, -1, N), e1234, out5), dim=1)
        assert tuple(concat.shape) == (B, 9025, N) and torch.equal(model.head(concat), logits)
        assert torch.equal(model(x, l.unsqueeze(1), idx=idx), logits)             # l as the reference's [B,1,16]
    st = {"pos": pos, "out1": out1, "out2": out2, "out3": out3, "out4": out4, "fstn": g, "h": h, "trans": frame, "e1234": e1234, "logits": logits}
    return {"out:" + key: P.recorded(key, v.numpy()) for key, v in st.items()}


def test_reference_state_loads_strictly_and_the_model_reproduces_the_recorded_run():
    """The reference's state_dict layout loads with strict=True, and the model on the recorded list reproduces every recorded stage and
    the logits.  The siblings' tolerance is kept, 1e-3 under compare_case, for their reason: torch.cross on an expanded view and the
    einsum's choice of a product need not round as the reference's do.  Worst value found while writing this (torch on the CPU): 0
    for every key."""
    import svnet_amd.models as M
    seed, B, N, k, num_part = P.GOLDEN_CASE
    model = PC.golden_model()
    assert isinstance(model, M.VN_PointNet_PSEG) and list(model.state_dict()) == [str(key) for key in GOLDEN["keys"]]
    assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(int(d) for d in s if d >= 0) for s in GOLDEN["shapes"]]
    assert model.k == k and model.num_part == num_part and model.fstn.d == 42 and tuple(model.convs1.weight.shape) == (256, 9025, 1)
    got = _model_stages(model, torch.from_numpy(GOLDEN["x"]), torch.from_numpy(GOLDEN["l"]), torch.from_numpy(GOLDEN["idx"]))
    assert sorted(got) == sorted("out:" + key for key in P.STAGES) and got["out:logits"].shape == (B, num_part, N)
    worst = compare_case(got, {key: GOLDEN[key[4:]] for key in got}, 1e-3, "the model against the recorded run")
    print("worst relative error %.3e at %s" % worst)
    x, l, idx = (torch.from_numpy(GOLDEN[key]) for key in ("x", "l", "idx"))
    with pytest.raises(ValueError, match="one neighbour list"):
        model(x, l, idx=[idx])
    with pytest.raises(ValueError, match=r"l must be \[B,16\]"):
        model(x, l[:, :8], idx=idx)


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_model_constructs_and_runs_in_both_poolings_and_in_train_mode(pooling):
    import svnet_amd.models as M
    B, N, k, num_part = 2, 12, 4, 7
    torch.manual_seed(3)
    model = M.VN_PointNet_PSEG(argparse.Namespace(k=k, pooling=pooling), num_part)
    keys = list(model.state_dict())
    assert ("pool.map_to_dir.weight" in keys) == ("fstn.pool.map_to_dir.weight" in keys) == (pooling == "max")
    x = torch.from_numpy(synth.cloud_batch(3, 0, 0, B, N))
    l = torch.from_numpy(synth.category_onehot(3, 0, 0, B))
    idx = torch.from_numpy(synth.integers(3, 1, (B, N, k), N))
    model.train()
    out = model(x, l, idx=idx)
    assert tuple(out.shape) == (B, num_part, N) and out.requires_grad and bool(torch.isfinite(out).all())
    out.square().mean().backward()
    # (a VNMaxPool's direction only selects: it takes no gradient)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for name, p in model.named_parameters() if "pool." not in name)
    assert int(model.bns1.num_batches_tracked) == 1 and int(model.bn5.bn.num_batches_tracked) == 1
    model.eval()
    with torch.no_grad():
        a, b = model(x, l, idx=idx), model(x, l, idx=idx)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="pooling"):
        M.VN_PointNet_PSEG(argparse.Namespace(k=k, pooling="sum"))


def test_restatement_of_the_fused_forward_equals_the_recorded_stages_and_logits():
    """The chained restatement - tests/vn_tail_ref.py, tests/vn_pointnet_ref.py and tests/vn_pseg_ref.py functions, the head in
    float64 - against every recorded stage within 1e-4 and the recorded logits within 1e-3."""
    got = PC.restated()
    seed, B, N, k, num_part = P.GOLDEN_CASE
    assert got["local"].shape == (B, P.WIDE, 3, N) and got["e5"].shape == (B, 3 * P.WIDE, N) and got["h"].shape == (B, P.POOLED)
    assert all(v.dtype == F32 for key, v in got.items() if key != "logits")
    # the amax half of the pool is the maximum of the per-point coordinates, of the local channels and of the mean's
    assert np.array_equal(got["h"][:, :3 * P.WIDE], got["e5"].max(-1))
    for key in P.STAGES:
        worst = compare_case({"out": P.recorded(key, got[key])}, {"out": GOLDEN[key]}, 1e-3 if key == "logits" else 1e-4, "the restatement, %s" % key)
        print("%s: worst relative error %.3e" % (key, worst[0]))


def test_wide_predicates_and_workspaces():
    from svnet_amd import vn_tail as VT
    L = _lib.lib()
    assert (VT.MAX_C, VT.MAX_O, VT.MAX_C_WIDE, VT.MAX_O_WIDE) == (512, 512, 768, 768)
    Q = VT.supported_point_wide                                                   # (N, C, Cg, O, Od)
    assert Q(16, 768, 768, 768, 768) and Q(16, 768, 768, 768, 1) and Q(32768, 1, 0, 1, 1) and Q(16, 4, 0, 4, 4)
    assert not Q(16, 769, 0, 4, 4) and not Q(16, 4, 769, 4, 4) and not Q(16, 4, 0, 769, 769) and not Q(16, 4, 0, 769, 1) and not Q(32769, 4, 0, 4, 4)
    assert not Q(0, 4, 0, 4, 4) and not Q(16, 0, 0, 4, 4) and not Q(16, 4, 0, 0, 0) and not Q(-1, 4, 0, 4, 4) and not Q(16, -1, 0, 4, 4)
    assert not Q(16, 4, -1, 4, 4) and not Q(16, 4, 0, -1, -1) and Q(16, 4, 0, 4, 1)
    assert not Q(16, 4, 0, 4, 2) and not Q(16, 4, 0, 4, 0) and not Q(16, 4, 0, 682, 341)          # Od neither O nor 1
    assert all(Q(N, 682, 682, 682, 682) for N in (1, 64, 2048, 32768))
    assert Q(16, 5, 0, 3, 3) == VT.supported_point(16, 5, 0, 3, 3, wide=True) and not VT.supported_point(16, 513, 0, 4, 4, wide=False)
    K = VT.supported_point_norm_wide                                              # (N, C, O)
    assert K(16, 768, 768) and K(2048, 170, 682) and not K(16, 769, 4) and not K(16, 4, 769) and not K(16, 0, 4) and not K(16, 4, 0)
    assert not K(0, 4, 4) and not K(-1, 4, 4) and not K(16, -1, 4) and not K(16, 4, -1) and not K(32769, 4, 4)
    S = VT.supported_std_wide                                                     # (N, C, Cg, Cy)
    assert S(16, 768, 768, 768) and S(2048, 682, 682, 341) and S(16, 4, 0, 4)
    assert not S(16, 769, 0, 4) and not S(16, 4, 769, 4) and not S(16, 4, 0, 769) and not S(0, 4, 0, 4) and not S(16, 0, 0, 4) and not S(16, 4, 0, 0)
    assert not S(-1, 4, 0, 4) and not S(16, -1, 0, 4) and not S(16, 4, -1, 4) and not S(16, 4, 0, -1) and not S(32769, 4, 0, 4)
    E = VT.supported_coords_wide                                                  # (N, C, Cy)
    assert E(16, 768, 768) and E(2048, 682, 341) and not E(16, 769, 4) and not E(16, 4, 769) and not E(16, 0, 4) and not E(16, 4, 0) and not E(0, 4, 4)
    assert not E(-1, 4, 4) and not E(16, -1, 4) and not E(16, 4, -1)
    # the old predicates beside them: 513 is refused as before
    assert VT.supported_point(16, 512, 512, 512, 1) and not VT.supported_point(16, 513, 0, 4, 4) and not VT.supported_point(16, 4, 513, 4, 4)
    assert not VT.supported_point(16, 4, 0, 513, 513)
    assert VT.supported_point_norm(16, 512, 512) and not VT.supported_point_norm(16, 513, 4) and not VT.supported_point_norm(16, 4, 513)
    assert VT.supported_std(16, 512, 512, 512) and not VT.supported_std(16, 513, 0, 4) and not VT.supported_std(16, 4, 513, 4) and not VT.supported_std(16, 4, 0, 513)
    assert VT.supported_coords(16, 512, 512) and not VT.supported_coords(16, 513, 4) and not VT.supported_coords(16, 4, 513)
    assert L.svnet_vn_point_workspace_bytes(2, 513, 4, 4) == 0 and L.svnet_vn_std_pool_workspace_bytes(2, 64, 513, 0) == 0
    # the wide workspaces at the model's widths, by the header's formulas: 3 B (O + Od) floats; 2 ceil(N / 64) B 3 (C + Cg) floats
    Bc, N = 32, 2048
    assert L.svnet_vn_point_wide_workspace_bytes(Bc, 682, 682, 682) == 3 * Bc * (682 + 682) * 4
    assert L.svnet_vn_point_wide_workspace_bytes(Bc, 0, 341, 341) == 0 and L.svnet_vn_point_wide_workspace_bytes(Bc, 768, 768, 1) == 3 * Bc * 769 * 4
    assert L.svnet_vn_point_wide_workspace_bytes(Bc, 769, 4, 4) == 0 and L.svnet_vn_point_wide_workspace_bytes(65536, 4, 4, 4) == 0
    assert L.svnet_vn_point_wide_workspace_bytes(0, 4, 4, 4) == 0
    assert L.svnet_vn_std_pool_wide_workspace_bytes(Bc, N, 682, 682) == 2 * (N // 64) * Bc * 3 * 1364 * 4
    assert L.svnet_vn_std_pool_wide_workspace_bytes(2, 65, 682, 682) == 2 * 2 * 2 * 3 * 1364 * 4
    assert L.svnet_vn_std_pool_wide_workspace_bytes(65535, 32768, 768, 768) == 2 * 512 * 65535 * 3 * 1536 * 4          # (no 32-bit overflow)
    assert L.svnet_vn_std_pool_wide_workspace_bytes(2, 64, 769, 0) == 0 and L.svnet_vn_std_pool_wide_workspace_bytes(2, 0, 4, 0) == 0
    # inside the base envelope the two agree
    assert L.svnet_vn_point_wide_workspace_bytes(3, 5, 7, 1) == L.svnet_vn_point_workspace_bytes(3, 5, 7, 1) == 3 * 3 * 8 * 4
    assert L.svnet_vn_std_pool_wide_workspace_bytes(3, 130, 5, 5) == L.svnet_vn_std_pool_workspace_bytes(3, 130, 5, 5)


def test_header_names_the_wide_entries_under_abi_437_and_they_refuse_769():
    header = open(_lib.HEADER_PATH).read()
    abi = int(re.search(r"#define SVNET_ABI_VERSION (\d+)", header).group(1))
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION == abi >= 437
    assert "437: " + ", ".join(WIDE_NAMES) in header and "THE NAMING RULE" in header and "1 <= C, O, Cy <= 768, 0 <= Cg <= 768" in header
    for name in WIDE_NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_wide", "")], name      # a twin has its entry's arguments
    L = _lib.lib()
    p = _lib.c_p(64)                                                              # refused before any launch: no device is touched
    E = _lib.DEFINES
    U, A = E["SVNET_E_UNSUPPORTED"], E["SVNET_E_ARG"]
    assert L.svnet_vn_point_wide_f32(p, p, p, 1, 16, 769, 0, 4, 4, 0.0, p, 64, p, None) == U
    assert b"svnet_vn_point_wide_f32" in L.svnet_last_error() and b"768" in L.svnet_last_error()
    assert L.svnet_vn_point_wide_f32(p, p, p, 1, 16, 4, 769, 4, 4, 0.0, p, 64, p, None) == U
    assert L.svnet_vn_point_wide_f32(p, p, p, 1, 16, 4, 0, 769, 769, 0.0, p, 64, p, None) == U
    assert L.svnet_vn_point_wide_f32(p, p, p, 1, 16, 4, 0, 8, 4, 0.0, p, 64, p, None) == U
    assert L.svnet_vn_point_wide_f32(None, p, p, 1, 16, 4, 0, 4, 4, 0.0, p, 64, p, None) == A
    assert L.svnet_vn_point_wide_f32(p, p, p, 65536, 16, 4, 0, 4, 4, 0.0, p, 64, p, None) == A
    assert L.svnet_vn_point_wide_f32(p, p, p, 2, 16, 4, 4, 4, 4, 0.0, p, 8, p, None) == E["SVNET_E_WORKSPACE"]
    assert L.svnet_vn_point_wide_fold_f32(p, p, p, p, p, p, 769, 0, 4, 4, 1e-5, p, None) == U
    assert L.svnet_vn_point_norm_wide_f32(p, p, 1, 16, 769, 4, p, None) == U and b"svnet_vn_point_norm_wide_f32" in L.svnet_last_error()
    assert L.svnet_vn_point_norm_wide_f32(p, p, 1, 16, 4, 769, p, None) == U and L.svnet_vn_point_norm_wide_f32(p, None, 1, 16, 4, 4, p, None) == A
    assert L.svnet_vn_point_norm_wide_fold_f32(p, p, p, p, p, 4, 769, 1e-5, p, None) == U
    assert L.svnet_vn_cloud_mean_wide_f32(p, 1, 769, 16, p, None) == U and b"svnet_vn_cloud_mean_wide_f32" in L.svnet_last_error()
    assert L.svnet_vn_cloud_mean_wide_f32(p, 1, 4, 32769, p, None) == U and L.svnet_vn_cloud_mean_wide_f32(p, 0, 4, 16, p, None) == A
    for C, Cg, Cy in ((769, 0, 4), (4, 769, 4), (4, 0, 769)):
        assert L.svnet_vn_std_pool_wide_f32(p, p, p, p, 1, 16, C, Cg, Cy, p, 1 << 20, p, None) == U
    assert b"svnet_vn_std_pool_wide_f32" in L.svnet_last_error()
    assert L.svnet_vn_std_pool_wide_f32(p, p, p, p, 1, 16, 4, 0, 4, p, 8, p, None) == E["SVNET_E_WORKSPACE"]
    assert L.svnet_vn_std_coords_wide_f32(p, p, p, 1, 16, 769, 4, p, None) == U and L.svnet_vn_std_coords_wide_f32(p, p, p, 1, 16, 4, 769, p, None) == U
    assert b"svnet_vn_std_coords_wide_f32" in L.svnet_last_error() and L.svnet_vn_std_coords_wide_f32(p, p, None, 1, 16, 4, 4, p, None) == A
    # the old entries still refuse 513, and say 512
    assert L.svnet_vn_point_f32(p, p, p, 1, 16, 513, 0, 4, 4, 0.0, p, 64, p, None) == U and b"512" in L.svnet_last_error()
    assert L.svnet_vn_point_norm_f32(p, p, 1, 16, 513, 4, p, None) == U
    assert L.svnet_vn_cloud_mean_f32(p, 1, 513, 16, p, None) == U
    assert L.svnet_vn_std_pool_f32(p, p, p, p, 1, 16, 513, 0, 4, p, 1 << 20, p, None) == U
    assert L.svnet_vn_std_coords_f32(p, p, p, 1, 16, 513, 4, p, None) == U


def test_fronts_refuse_the_wide_widths_unless_asked_and_name_the_envelope():
    """The opt-in is explicit: without wide=True a 682-wide layer is refused as before, with the base envelope in the message; the
    checks of the arguments come first and need no device."""
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.vn_layers import VNBatchNorm, VNLinear, VNLinearLeakyReLU
    for wide in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                # (the device question comes before the envelope's)
            VT.fold_vn_point(VNLinearLeakyReLU(4, 5), wide=wide)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            VT.fold_vn_linear_norm(VNLinear(4, 5), VNBatchNorm(5, dim=4), wide=wide)
    fp = VC.fake(VT.FoldedVNPoint, C=3, Cg=0, O=5, Od=5)
    assert fp.wide is False and VC.fake(VT.FoldedVNPointNorm, C=3, O=5).wide is False
    x = torch.zeros(2, 3, 3, 16)
    for kw in ({}, {"wide": True}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            VT.vn_cloud_mean(x, **kw)
        with pytest.raises(ValueError, match=r"w_lin must be \[3,Cy\]"):
            VT.vn_std_coords(x, torch.zeros(2, 4, 3, 16), torch.zeros(3, 5), **kw)
        with pytest.raises(ValueError, match="cloud must be"):
            VT.vn_std_pool(x, torch.zeros(2, 4, 3, 16), torch.zeros(3, 4), cloud=torch.zeros(2, 3), **kw)
    assert VT._entry("point", "f32", False) == "svnet_vn_point_f32" and VT._entry("std_pool", "workspace_bytes", True) == "svnet_vn_std_pool_wide_workspace_bytes"
    assert VT._widest(False) == (512, 512) and VT._widest(True) == (768, 768)


def test_wrapper_refuses_what_it_cannot_take():
    from svnet_amd import vn_pointnet_pseg as VP
    from tests import vn_pointnet_cases as CLS
    with pytest.raises(TypeError, match="VN_PointNet_PSEG"):
        VP.FusedVNPointNetPSeg(CLS.golden_model())                                # (the PointNet classifier)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VP.FusedVNPointNetPSeg(PC.golden_model())
    # pooling = 'max' and normalize_frame: nothing to fold, so the wrapper lives on the CPU too; every call is the model's
    framed = PC.golden_model()
    framed.std_feature.normalize_frame = True
    x, l, idx = (torch.from_numpy(GOLDEN[key]) for key in ("x", "l", "idx"))
    for model in (PC.golden_model(pooling="max"), framed):
        fused = VP.FusedVNPointNetPSeg(model)
        assert not fused.fused and fused.cross is None and not fused.points and not fused.supported(2, 64, 8)
        VC.cpu_wrapper_refuses(fused, (x, l), [
            (TypeError, "x must be torch.float32", (x.double(), l), {}),
            (ValueError, "x requires grad", (x.clone().requires_grad_(), l), {}),
            (ValueError, r"x must be \[B,3,N\]", (x[:, :2].contiguous(), l), {}),
            (ValueError, "neighbour list", (x, l), {"idx": [idx]}),
            (ValueError, r"l must be \[B,16\]", (x, l[:, :8].contiguous()), {"idx": idx}),
            (RuntimeError, "no CPU fallback", (x, l), {"idx": idx})])
