"""The fused binary chain (svnet_amd/csrc/bi_chain.hip, svnet_amd/bi_fused.py) and FusedBiPointNet on the GPU.  Everything is compared
as bit patterns against the numpy restatement tests/bi_ref.py, a -0 counted as +0; the cases take explicit offsets, so N is free.
The shapes are the smallest at which the kernel can go wrong: the tile edges (R = rows_tile), the cross-tile maximum, the separation of
clouds, widths around the 32-wide MFMA blocks and k-steps and the 128-wide groups of four, and the limits themselves."""
import types

import numpy as np
import pytest
import torch

from svnet_amd import _lib, bi_fused as F
from svnet_amd.models.bipointnet import BasicBiPointNet, BiPointNetLSREMax
from svnet_amd.models.bipointnet_basic import BiLinearLSR
from tests import bi_ref as R
from tests.common import compare_case, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make_bi(rng, K, O, bn=True, W=None, scale=None, gamma=None, beta=None, mean=None, var=None, eps=1e-5):
    """A BiLinearLSR K -> O and its BatchNorm1d (None without bn) on the device, with the given arrays or random ones -> (lin, norm)."""
    lin = BiLinearLSR(K, O)
    W = (rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32) if W is None else np.asarray(W, dtype=np.float32)
    lin.weight.data = _t(W)
    lin.scale.data = torch.tensor(float(rng.uniform(0.02, 0.08)) if scale is None else float(scale), dtype=torch.float32)
    norm = None
    if bn:
        norm = torch.nn.BatchNorm1d(O, eps=eps)
        sign = np.where(rng.integers(0, 2, O) == 0, 1.0, -1.0)
        norm.weight.data = _t((rng.uniform(0.5, 1.5, O) * sign if gamma is None else np.asarray(gamma)).astype(np.float32))
        norm.bias.data = _t((0.2 * rng.standard_normal(O) if beta is None else np.asarray(beta)).astype(np.float32))
        norm.running_mean.data = _t((0.25 * rng.standard_normal(O) if mean is None else np.asarray(mean)).astype(np.float32))
        norm.running_var.data = _t((rng.uniform(0.5, 1.5, O) if var is None else np.asarray(var)).astype(np.float32))
        norm = norm.to(DEV).eval()
    return lin.to(DEV).eval(), norm


def make_fp(rng, K, O):
    lin = torch.nn.Linear(K, O)
    lin.weight.data = _t((rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32))
    lin.bias.data = _t((0.1 * rng.standard_normal(O)).astype(np.float32))
    _, norm = make_bi(rng, K, O)
    return lin.to(DEV).eval(), norm


def _np(t):
    return t.detach().cpu().numpy()


def _stats(norm):
    return None if norm is None else (_np(norm.weight), _np(norm.bias), _np(norm.running_mean), _np(norm.running_var), norm.eps)


def both(pairs, first_fp):
    """[(lin, norm)] -> (the folded layers on the device, the restatement's layers)."""
    dev, ref = [], []
    for i, (lin, norm) in enumerate(pairs):
        if i == 0 and first_fp:
            dev.append(F.fold_fp_layer(lin, norm))
            ref.append(("fp",) + tuple(R.fold_fp(_np(lin.weight), _np(lin.bias), _stats(norm))))
        else:
            dev.append(F.fold_bi_layer(lin, norm))
            ref.append(("bi", R.fold_bi(_np(lin.weight), _np(lin.scale), _stats(norm))))
    return dev, ref


def random_chain(rng, C0, widths, first_fp, scale=None):
    pairs, k = [], C0
    for i, o in enumerate(widths):
        pairs.append(make_fp(rng, k, o) if i == 0 and first_fp else make_bi(rng, k, o, scale=scale))
        k = o
    return both(pairs, first_fp)


def check(x, dev, ref, trans=None, epilogues=("write", "max"), offset=-0.75, clamp=True):
    """The kernel against the restatement on x [B,C0,N] (numpy), for both epilogues; -> {epilogue: the restatement's result}."""
    xd = _t(x).to(DEV)
    td = None if trans is None else _t(trans).to(DEV)
    out = {}
    for ep in epilogues:
        pool = "max" if ep == "max" else None
        got = _np(F.bi_chain(xd, dev, trans=td, pool=pool, offset=offset, clamp=clamp))
        want = R.chain(x, ref, trans=trans, pool=pool, offset=offset, clamp=clamp)
        assert got.shape == want.shape
        bad = R.positive_zero(got) != R.positive_zero(want)
        assert not bad.any(), "%s: %d of %d values differ, first at %s: %r against %r" % (
            ep, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])
        out[ep] = want
    return out


def cloud(rng, B, C0, N):
    return rng.standard_normal((B, C0, N)).astype(np.float32)


def test_fold_matches_the_restatement_bit_for_bit():
    rng = np.random.default_rng(1)
    for K, O, bn in ((128, 1024, True), (1024, 512, True), (256, 9, False), (3, 5, True)):
        lin, norm = make_bi(rng, K, O, bn=bn)
        f = F.fold_bi_layer(lin, norm)
        want = R.fold_bi(_np(lin.weight), _np(lin.scale), _stats(norm))
        ab = _np(f.ab)
        assert np.array_equal(R.positive_zero(ab[:O]), R.positive_zero(want["a"])) and np.array_equal(R.positive_zero(ab[O:]), R.positive_zero(want["b"]))
        assert np.array_equal(_np(f._s), want["S"].astype(np.float32))
        if K <= 512:
            Kp, Op = (K + 31) // 32 * 32, (O + 31) // 32 * 32
            packed = _np(f.w_i8).reshape(Op, Kp)
            assert np.array_equal(packed[:O, :K], want["S"]) and not packed[O:].any() and not packed[:, K:].any()
        else:
            assert f.w_i8 is None


@pytest.mark.parametrize("dn", [None, -1, 0, 1, "2R+2"])
def test_tile_edges_cross_tile_maximum_and_cloud_separation(dn):
    Rt = F.rows_tile()
    N = 1 if dn is None else (2 * Rt + 2 if dn == "2R+2" else Rt + dn)
    rng = np.random.default_rng(N)
    dev, ref = random_chain(rng, 3, [16, 40, 70], True)
    check(cloud(rng, 3, 3, N), dev, ref)


@pytest.mark.parametrize("K", [1, 3, 63, 64, 65, 128, 130, 512])
def test_binary_input_widths(K):
    rng = np.random.default_rng(K)
    dev, ref = random_chain(rng, K, [33, 40], False)
    check(cloud(rng, 2, K, F.rows_tile() + 1), dev, ref)


@pytest.mark.parametrize("O", [1, 9, 127, 129, 1024, 2048])
def test_last_widths(O):
    rng = np.random.default_rng(O)
    dev, ref = random_chain(rng, 20, [O], False)
    check(cloud(rng, 2, 20, 130), dev, ref)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("first", ["fp1", "fp3", "fp9", "bi"])
def test_depths_and_first_layers(L, first):
    rng = np.random.default_rng(10 * L + len(first))
    C0 = int(first[2:]) if first != "bi" else 24
    dev, ref = random_chain(rng, C0, [48, 32, 96, 40][:L], first != "bi")
    check(cloud(rng, 2, C0, 70), dev, ref)


@pytest.mark.parametrize("C0,first_fp", [(3, True), (64, False), (64, True), (5, False)])
def test_transform_in_front(C0, first_fp):
    rng = np.random.default_rng(C0 + first_fp)
    dev, ref = random_chain(rng, C0, [64, 128], first_fp)
    trans = (np.eye(C0) + 0.3 * rng.standard_normal((2, C0, C0))).astype(np.float32)
    check(cloud(rng, 2, C0, 131), dev, ref, trans=trans)


@pytest.mark.parametrize("clamp", [True, False])
def test_write_clamps_on_both_sides_of_one(clamp):
    rng = np.random.default_rng(5)
    dev, ref = random_chain(rng, 16, [32, 24], False, scale=0.5)
    x = cloud(rng, 2, 16, 90)
    free = R.chain(x, ref, clamp=False)
    assert (free > 1).any() and (free < -1).any() and (np.abs(free) < 1).any()
    got = check(x, dev, ref, epilogues=("write",), clamp=clamp)["write"]
    assert (np.abs(got).max() <= 1) == clamp
    # the fp layer's write, as the encoder's conv1 uses it
    dev, ref = random_chain(rng, 3, [64], True)
    x3 = 3 * cloud(rng, 2, 3, 90)
    free = R.chain(x3, ref, clamp=False)
    assert (free > 1).any() and (free < -1).any()
    check(x3, dev, ref, epilogues=("write", "max"), clamp=clamp)


def test_maximum_with_positive_negative_and_zero_slopes_and_an_offset():
    rng = np.random.default_rng(6)
    O = 70
    gamma = rng.uniform(0.5, 1.5, O) * np.where(np.arange(O) % 3 == 0, 1, -1)
    gamma[1::7] = 0.0
    pairs = [make_bi(rng, 20, 36), make_bi(rng, 36, O, gamma=gamma)]
    dev, ref = both(pairs, False)
    a = ref[1][1]["a"]
    assert (a > 0).any() and (a < 0).any() and (a == 0).any()
    for offset in (0.0, -3.2041, 2.5):
        check(cloud(rng, 3, 20, 2 * F.rows_tile() + 5), dev, ref, epilogues=("max",), offset=offset)


def test_maximum_of_negative_values_only():
    """Every t negative: a maximum seeded with 0, or one that takes in the zero rows past N of the last tile, is caught."""
    rng = np.random.default_rng(7)
    pairs = [make_bi(rng, 12, 40, beta=np.full(40, -30.0))]
    dev, ref = both(pairs, False)
    x = cloud(rng, 2, 12, F.rows_tile() + 3)
    got = check(x, dev, ref, epilogues=("max",), offset=0.0)["max"]
    assert (got < 0).all()


def test_maximum_in_the_last_valid_row_below_what_the_padding_would_give():
    """K 4, one channel, W = c (+ + - -): m = 0.  Every real row has d < 0 and the largest, -2, is the cloud's last row, alone in its
    tile beside rows that were staged as zeros: those would give d = 0 > -2."""
    rng = np.random.default_rng(8)
    c = 0.37
    lin, norm = make_bi(rng, 4, 1, W=[[c, c, -c, -c]], scale=1.0, gamma=[1.0], beta=[0.25], mean=[0.0], var=[1.0], eps=0.0)
    dev, ref = both([(lin, norm)], False)
    assert ref[0][1]["m"] == 0 and ref[0][1]["a"][0] == 1
    N = F.rows_tile() + 1
    x = np.tile(np.array([-1.0, -2.0, 3.0, 0.5], dtype=np.float32)[None, :, None], (2, 1, N))        # d = -4
    x[:, :, -1] = np.array([-1.0, 2.0, 3.0, 0.5], dtype=np.float32)[None]                            # d = -2
    got = check(x, dev, ref, epilogues=("max",), offset=0.0)["max"]
    assert np.array_equal(got, np.full((2, 1), -1.75, dtype=np.float32))


def test_ternary_zeros_in_x_in_t_and_in_the_weights():
    rng = np.random.default_rng(9)
    # exact zeros planted in x, under a binary first layer and under a transform
    dev, ref = random_chain(rng, 9, [32, 16], False)
    x = cloud(rng, 2, 9, 75)
    x[rng.random(x.shape) < 0.3] = 0.0
    x[0, :, 5] = 0.0
    check(x, dev, ref)
    check(x, dev, ref, trans=np.tile(np.eye(9, dtype=np.float32), (2, 1, 1)))
    # a = 1, b = -d0: t == 0 occurs and the next layer reads a zero
    K, O, d0 = 8, 6, 2.0
    first = make_bi(rng, K, O, scale=1.0, gamma=np.ones(O), beta=np.full(O, -d0), mean=np.zeros(O), var=np.ones(O), eps=0.0)
    dev, ref = both([first, make_bi(rng, O, 12)], False)
    x = cloud(rng, 2, K, 200)
    t = R.chain(x, ref[:1], clamp=False)
    assert (t == 0).any() and (t > 0).any() and (t < 0).any()
    check(x, dev, ref)
    # weights from {-c, 0, +c} with balanced counts: m = 0 and the zeros stay zeros
    c = 0.21
    W = np.resize(np.array([c, 0.0, -c, 0.0, -c, c], dtype=np.float32), (10, 12))
    assert W.sum() == 0
    dev, ref = both([make_bi(rng, 12, 10, W=W)], False)
    assert ref[0][1]["m"] == 0 and (ref[0][1]["S"] == 0).sum() == 40
    check(cloud(rng, 2, 12, 40), dev, ref)
    # a constant W: every weight is 0, every count is 0
    dev, ref = both([make_bi(rng, 12, 10, W=np.full((10, 12), 0.125, dtype=np.float32))], False)
    assert not ref[0][1]["S"].any()
    check(cloud(rng, 2, 12, 40), dev, ref)


def test_two_runs_give_equal_bits_and_a_captured_graph_replays_the_eager_result():
    rng = np.random.default_rng(10)
    dev, _ = random_chain(rng, 3, [64, 128, 256], True)
    x = _t(cloud(rng, 3, 3, 2 * F.rows_tile() + 9)).to(DEV)
    one = F.bi_chain(x, dev, pool="max", offset=-1.0)
    two = F.bi_chain(x, dev, pool="max", offset=-1.0)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    ws = F._vn.Workspace(x.device)
    out = torch.empty_like(one)
    F.bi_chain(x, dev, pool="max", offset=-1.0, out=out, workspace=ws)       # (the workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for f in dev:
            f.refresh()
        F.bi_chain(x, dev, pool="max", offset=-1.0, out=out, workspace=ws)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), one.view(torch.int32))


# ---- the wrapper on the recorded case
@pytest.fixture(scope="module")
def golden():
    g = load_npz("bipointnet.npz")
    seed, B, N, num_class = R.GOLDEN_CASE
    state = R.synthetic_state(g["keys"], g["shapes"], seed)
    model = BiPointNetLSREMax(types.SimpleNamespace(), num_class)
    model.load_state_dict({k: _t(v) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval()
    want, signs = R.forward(g["x"], state)
    return g, state, model, want, signs


def test_wrapper_on_the_golden_case(golden):
    g, state, model, want, signs = golden
    fused = F.FusedBiPointNet(model)
    x = _t(g["x"]).to(DEV)
    B, N = x.shape[0], x.shape[2]
    assert fused.fused and fused.supported(B, N)
    st = fused.encode(x)
    logits, trans_feat = fused(x)
    assert torch.equal(logits, st["logits"]) and torch.equal(trans_feat, st["trans_feat"])
    assert torch.equal(F.FusedBiPointNet(model, logits_only=True)(x), logits)
    # bit-equal to the restatement up to each pooled tensor (and through the fully connected layers between them)
    for key in ("pool_stn", "trans", "h1", "pool_fstn", "trans_feat", "pool", "fc2"):
        assert np.array_equal(R.positive_zero(_np(st[key])), R.positive_zero(want[key])), key
    # within the project's tolerance of the reference's recorded run
    got = {"out:" + k: _np(st[k]) for k in R.STAGES}
    worst = compare_case(got, {"out:" + k: g[k] for k in R.STAGES}, 1e-3, "FusedBiPointNet")
    print("worst against the recorded run: %.3e at %s" % worst)
    # every recorded sign plane, from the device: chain prefixes written unclamped, and the inputs of the fully connected layers
    C = fused.chains
    rows = lambda t: _np(t.permute(0, 2, 1).reshape(B * N, -1))       # noqa: E731
    planes = {
        "feat.stn.conv2.lin": rows(F.bi_chain(x, C["A"][:1], clamp=False)),
        "feat.stn.conv3.lin": rows(F.bi_chain(x, C["A"][:2], clamp=False)),
        "feat.fstn.conv1.lin": rows(st["h1"]),
        "feat.fstn.conv2.lin": rows(F.bi_chain(st["h1"], C["C"][:1], clamp=False)),
        "feat.fstn.conv3.lin": rows(F.bi_chain(st["h1"], C["C"][:2], clamp=False)),
        "feat.conv3.lin": rows(F.bi_chain(st["h1"], C["D"][:1], trans=st["trans_feat"], clamp=False)),
        "feat.stn.fc1": _np(st["pool_stn"]), "feat.fstn.fc1": _np(st["pool_fstn"]), "fc1": _np(st["pool"]),
    }
    for key, pool in (("feat.stn.", "pool_stn"), ("feat.fstn.", "pool_fstn"), ("", "pool")):
        group = fused.fcs[{"feat.stn.": "stn", "feat.fstn.": "fstn", "": "head"}[key]]
        h = group[0].linear_rows(st[pool])
        planes[key + "fc2"] = _np(h)
        if len(group) > 2:
            planes[key + "fc3"] = _np(group[1].linear_rows(h))
    # feat.conv2's input is bmm(h1^T, trans_feat), the chain's transform: an identity fp layer behind it writes u itself
    eye = torch.nn.Linear(64, 64)
    eye.weight.data, eye.bias.data = torch.eye(64), torch.zeros(64)
    unit = torch.nn.BatchNorm1d(64, eps=0.0)
    planes["feat.conv2.lin"] = rows(F.bi_chain(st["h1"], [F.fold_fp_layer(eye.to(DEV), unit.to(DEV).eval())], trans=st["trans_feat"], clamp=False))
    assert sorted(planes) == sorted(R.BI_LAYERS)
    for key in R.BI_LAYERS:
        rec = R.unpack_signs(g["sp:" + key], g["sz:" + key], signs[key].shape[1])
        assert np.array_equal(signs[key], rec), key                      # the restatement
        assert np.array_equal(R.sgn(planes[key]), rec), key              # the device


def test_wrapper_falls_back_and_refuses_train_mode(golden):
    g, state, model, want, signs = golden
    x = _t(g["x"]).to(DEV)
    seed, B, N, num_class = R.GOLDEN_CASE
    # bi_last: the head's fc3 is binary -> the model's own forward
    other = BasicBiPointNet(k=num_class, Linear=BiLinearLSR, pool="ema-max", bi_last=True).to(DEV).eval()
    with torch.no_grad():
        ref = other(x)                                                  # (sets every scale)
    fused = F.FusedBiPointNet(other)
    assert not fused.fused and not fused.supported(B, N)
    got = fused(x)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # a scale of 0: not folded, the model runs (and sets it)
    fresh = BiPointNetLSREMax(types.SimpleNamespace(), num_class).to(DEV).eval()
    fused = F.FusedBiPointNet(fresh)
    assert not fused.fused
    assert fused(x)[0].shape == (B, num_class) and float(fresh.fc1.scale.detach()) != 0.0
    with pytest.raises(ValueError, match="reset_scale"):
        F.fold_bi_layer(BiLinearLSR(8, 8).to(DEV))
    # N outside offset_map: the model's KeyError
    with pytest.raises(KeyError):
        F.FusedBiPointNet(model)(x[:, :, :512].contiguous())
    # train mode
    wrapper = F.FusedBiPointNet(model)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="train mode"):
            wrapper(x)
    finally:
        model.eval()
    with pytest.raises(_lib.SvnetHipError, match="not supported"):
        F.bi_chain(torch.zeros(1, 3, 40000, device=DEV), wrapper.chains["A"])
