"""GPU tests (-m gpu): every dispatch tier of the layer kernels against a plain float64 restatement of the operation.

tests/golden/harness.py's op cases run each layer at toy sizes (2-63 rows, C <= 37, a pooled axis of 5-6), so every kernel below takes
only the smallest branch of its dispatch there; at production sizes the same kernels were only compared indirectly (model-level tests
with replayed decisions, fused-vs-layer-wise tests that compare HIP with HIP).  Here each family is called through the product's own
entry point (the _ops autograd Function or the sv_layers module the models call) at shapes on both sides of every dispatch boundary,
at ragged sizes and at sizes past the grid caps, and compared - forward and, through a seeded random upstream gradient, every input
and parameter gradient - with the textbook operation written below in float64 on the CPU.

Bounds: values that do not depend on a summation order (max, copies, subtractions, arg-max) are bit-exact; everything else goes through
tests/common.py:compare_case at OUT_RTOL (forward values, running statistics) and GRAD_RTOL (gradients) of the tensor's max.  Each family
has a teeth check: one element of the HIP output off by one part in 1e4 (or one arg-max moved) must fail the same comparison.

The classifier's fused vector tail (csrc/vtail.hip) has a section of the same kind; its reference is the oracle's own chain in float64 on
the HIP run's replayed, certified arg-max (tests/vtail_cases.py), because near-ties between float32 results are not a rule to pin.
"""
import numpy as np
import pytest
import torch

from tests.common import compare_case

pytestmark = pytest.mark.gpu

OUT_RTOL = 1e-5         # forward values and running statistics, relative to the tensor's max
GRAD_RTOL = 1e-4        # gradients
STE_CLIP = 1.2          # sv_layers.py: the clamp of the binarized weights' straight-through estimator
F64 = torch.float64


def _gen(*key):
    """A generator seeded from the case's key (stable across runs and hosts, unlike hash())."""
    s = 0
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(s)


def _np(t):
    return t.detach().cpu().numpy()


def check(got, ref, exact=(), name=""):
    """exact keys bit for bit; the rest with compare_case: 'out*' / 'buf:*' keys at OUT_RTOL, gradients at GRAD_RTOL."""
    for k in exact:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, "%s/%s: shape %s vs %s" % (name, k, g.shape, r.shape)
        bad = np.flatnonzero(g.ravel() != r.ravel())
        assert bad.size == 0, "%s/%s: %d elements differ, first at %d: %r vs %r" % (name, k, bad.size, bad[0], g.ravel()[bad[0]], r.ravel()[bad[0]])
    fwd = {k: v for k, v in ref.items() if k not in exact and (k.startswith("out") or k.startswith("buf:"))}
    bwd = {k: v for k, v in ref.items() if k not in exact and k not in fwd}
    worst = [0.0, 0.0]
    if fwd:
        worst[0] = compare_case(got, fwd, OUT_RTOL, name)[0]
    if bwd:
        worst[1] = compare_case(got, bwd, GRAD_RTOL, name)[0]
    return worst


def teeth(got, ref, exact=(), name="", key=None):
    """The comparison must fail once one element of a forward output moves by one part in 1e4."""
    check(got, ref, exact, name)
    key = key or next(k for k in ref if k.startswith("out"))
    bad = dict(got)
    bad[key] = np.array(got[key], dtype=np.float32, copy=True)
    i = int(np.abs(bad[key]).argmax())
    bad[key].flat[i] = bad[key].flat[i] * np.float32(1.0 + 1e-4) if bad[key].flat[i] != 0 else np.float32(1e-4)
    with pytest.raises(AssertionError):
        check(bad, ref, exact, "teeth:" + name)


def _leaf(t, dev):
    return t.to(dev).requires_grad_(True)


def _ste_sign(W):
    """sign(W) forward, clamp(-1.2, 1.2)'s gradient backward (sv_layers.py:44-48, the exact form)."""
    Wc = torch.clamp(W, -STE_CLIP, STE_CLIP)
    return torch.sign(Wc).detach() + (Wc - Wc.detach())


# ----------------------------------------------------------------------------- Vector2Scalar / V2SCat / VProject (csrc/v2s.hip)
# v2s_fwd/bwd_kernel<G, CPL>: C <= 3 -> <1,3>, <= 24 -> <8,3>, <= 96 -> <32,3>, <= 192 -> <64,3>, <= 384 -> <64,6>, <= 768 -> <64,12>
# (vproject: the same from <8,3> up).  v2s_grid caps at 2048 workgroups of 4 * 256 / G rows: G = 64 strides past 32 768 rows.

V2S_C = [3, 4, 24, 25, 96, 97, 192, 193, 384, 385, 768]


def _v2s_rows(C):
    return 1001 if C <= 96 else 333


def _v2s_inputs(tag, M, C, Cs=0, binary=False):
    g = _gen("v2s", tag, M, C, Cs, binary)
    v = torch.randn(M, 3, C, generator=g)
    W = torch.randn(3, C, generator=g) * (0.9 if binary else 0.3)
    sc = (torch.rand(1, 3, generator=g) + 0.5) / C ** 0.5 if binary else None
    s = torch.randn(M, Cs, generator=g) if Cs else None
    gs = torch.randn(M, Cs + 3 * C, generator=g)
    gz = torch.randn(M, 3, 3, generator=g)
    return v, W, sc, s, gs, gz


def _w_eff64(W, sc):
    return W if sc is None else _ste_sign(W) * sc.view(3, 1)


def run_v2s(M, C, binary, dev, tag="v2s"):
    from svnet_amd import _ops
    v, W, sc, _, gs, gz = _v2s_inputs(tag, M, C, 0, binary)
    vd, Wd = _leaf(v, dev), _leaf(W, dev)
    scd = _leaf(sc, dev) if binary else None
    s, z = _ops.V2S.apply(vd, Wd, scd, True)
    torch.autograd.backward([s, z], [gs.to(dev), gz.to(dev)])
    got = {"out0": _np(s), "out1": _np(z), "dx0": _np(vd.grad), "d:W": _np(Wd.grad)}
    v6, W6 = v.double().requires_grad_(True), W.double().requires_grad_(True)
    sc6 = sc.double().requires_grad_(True) if binary else None
    z6 = torch.einsum("mic,jc->mij", v6, _w_eff64(W6, sc6))
    s6 = torch.einsum("mic,mij->mcj", v6, z6).reshape(M, 3 * C)
    torch.autograd.backward([s6, z6], [gs.double(), gz.double()])
    ref = {"out0": _np(s6), "out1": _np(z6), "dx0": _np(v6.grad), "d:W": _np(W6.grad)}
    if binary:
        got["d:scale"], ref["d:scale"] = _np(scd.grad), _np(sc6.grad)
    return got, ref, ()


def run_v2scat(M, C, binary, dev, Cs=37, tag="v2scat"):
    from svnet_amd import _ops
    v, W, sc, s, gs, _ = _v2s_inputs(tag, M, C, Cs, binary)
    sd, vd, Wd = _leaf(s, dev), _leaf(v, dev), _leaf(W, dev)
    scd = _leaf(sc, dev) if binary else None
    cat = _ops.V2SCat.apply(sd, vd, Wd, scd, True)
    cat.backward(gs.to(dev))
    got = {"out0": _np(cat), "dx0": _np(sd.grad), "dx1": _np(vd.grad), "d:W": _np(Wd.grad)}
    s6, v6, W6 = s.double().requires_grad_(True), v.double().requires_grad_(True), W.double().requires_grad_(True)
    sc6 = sc.double().requires_grad_(True) if binary else None
    z6 = torch.einsum("mic,jc->mij", v6, _w_eff64(W6, sc6))
    cat6 = torch.cat([s6, torch.einsum("mic,mij->mcj", v6, z6).reshape(M, 3 * C)], dim=1)
    cat6.backward(gs.double())
    ref = {"out0": _np(cat6), "dx0": _np(s6.grad), "dx1": _np(v6.grad), "d:W": _np(W6.grad)}
    if binary:
        got["d:scale"], ref["d:scale"] = _np(scd.grad), _np(sc6.grad)
    # (the s columns are a copy, the s gradient a view of the incoming one: bit-exact)
    got["out_s"], ref["out_s"] = got["out0"][:, :Cs], s.numpy()
    return got, ref, ("out_s", "dx0")


def run_vproject(M, C, dev, tag="vproject"):
    from svnet_amd import _ops
    g = _gen(tag, M, C)
    v, z, gs = torch.randn(M, 3, C, generator=g), torch.randn(M, 3, 3, generator=g), torch.randn(M, 3 * C, generator=g)
    vd, zd = _leaf(v, dev), _leaf(z, dev)
    s = _ops.VProject.apply(vd, zd)
    s.backward(gs.to(dev))
    v6, z6 = v.double().requires_grad_(True), z.double().requires_grad_(True)
    s6 = torch.einsum("mic,mij->mcj", v6, z6).reshape(M, 3 * C)
    s6.backward(gs.double())
    return ({"out0": _np(s), "dx0": _np(vd.grad), "dx1": _np(zd.grad)},
            {"out0": _np(s6), "dx0": _np(v6.grad), "dx1": _np(z6.grad)}, ())


@pytest.mark.parametrize("binary", [False, True], ids=["fp", "bin"])
@pytest.mark.parametrize("C", V2S_C)
def test_v2s_tiers(C, binary, hip_device):
    check(*run_v2s(_v2s_rows(C), C, binary, hip_device), name="v2s C=%d" % C)


@pytest.mark.parametrize("binary", [False, True], ids=["fp", "bin"])
@pytest.mark.parametrize("C", V2S_C)
def test_v2scat_tiers(C, binary, hip_device):
    check(*run_v2scat(_v2s_rows(C), C, binary, hip_device), name="v2scat C=%d" % C)


@pytest.mark.parametrize("C", V2S_C)
def test_vproject_tiers(C, hip_device):
    check(*run_vproject(_v2s_rows(C), C, hip_device), name="vproject C=%d" % C)


@pytest.mark.parametrize("C", [25, 97, 193])
def test_v2s_grid_stride(C, hip_device):
    """More rows than 2048 workgroups cover in one sweep (G = 64: 32 768 rows; G = 32: 65 536), a ragged tail."""
    M = 65536 + 4097 if C <= 96 else 32768 + 4097
    check(*run_v2s(M, C, True, hip_device, tag="v2s_gs"), name="v2s grid-stride C=%d" % C)
    check(*run_vproject(M, C, hip_device, tag="vp_gs"), name="vproject grid-stride C=%d" % C)


def run_v2scat_sum(clouds, rows, C, Cs, dev):
    """V2SCat with the gate MLP inside: v2s_fwd_kernel<32 | 64, 3, true> copies s, sums its columns per cloud (fp64) and the gate MLP
    starts from those sums."""
    from svnet_amd import _ops, _lib
    M = clouds * rows
    assert _lib.lib().svnet_v2s_cat_sum_supported(M, C, Cs, rows) == 1
    v, W, sc, s, gs, _ = _v2s_inputs("v2scat_sum", M, C, Cs, True)
    g = _gen("v2scat_sum/gate", M, C, Cs)
    H, Ov = max(Cs // 3, 1), 2 * C // 3 + 1
    W0, W2 = torch.randn(H, Cs, generator=g) * 0.2, torch.randn(Ov, H, generator=g) * 0.2
    ggate = torch.randn(clouds, Ov, generator=g)
    sd, vd, Wd, scd, W0d, W2d = (_leaf(t, dev) for t in (s, v, W, sc, W0, W2))
    cat, gate = _ops.V2SCat.apply(sd, vd, Wd, scd, True, clouds, W0d, W2d)
    torch.autograd.backward([cat, gate], [gs.to(dev), ggate.to(dev)])
    got = {"out0": _np(cat), "out1": _np(gate), "dx0": _np(sd.grad), "dx1": _np(vd.grad), "d:W": _np(Wd.grad), "d:scale": _np(scd.grad),
           "d:W0": _np(W0d.grad), "d:W2": _np(W2d.grad)}
    s6, v6, W6, sc6, W06, W26 = (t.double().requires_grad_(True) for t in (s, v, W, sc, W0, W2))
    z6 = torch.einsum("mic,jc->mij", v6, _w_eff64(W6, sc6))
    cat6 = torch.cat([s6, torch.einsum("mic,mij->mcj", v6, z6).reshape(M, 3 * C)], dim=1)
    gate6 = torch.sigmoid(torch.relu(s6.view(clouds, rows, Cs).mean(1) @ W06.t()) @ W26.t())
    torch.autograd.backward([cat6, gate6], [gs.double(), ggate.double()])
    ref = {"out0": _np(cat6), "out1": _np(gate6), "dx0": _np(s6.grad), "dx1": _np(v6.grad), "d:W": _np(W6.grad), "d:scale": _np(sc6.grad),
           "d:W0": _np(W06.grad), "d:W2": _np(W26.grad)}
    return got, ref, ()


@pytest.mark.parametrize("cfg", [(3, 96, 25, 200), (2, 480, 96, 256), (4, 64, 97, 300), (2, 1008, 192, 512)],
                         ids=["G32_C25", "G32_C96", "G64_C97", "G64_C192"])
def test_v2scat_sum_tiers(cfg, hip_device):
    clouds, rows, C, Cs = cfg
    check(*run_v2scat_sum(clouds, rows, C, Cs, hip_device), name="v2scat_sum %r" % (cfg,))


# ----------------------------------------------------------------------------- pooling (csrc/pool.hip)
# pool_fwd: mean split for R >= 256, outer * inner < 2^20, outer <= 65535 (pool_mean_split_kernel + finish); max split with a key
# workspace (pool_max_split_kernel + unpack); pool_fwd_kernel otherwise.  pool_bwd: inner >= 128 and outer <= 65535 ->
# pool_maxmean_bwd_kernel, else pool_bwd_kernel.  pool_maxmean_fwd (one pass) for R >= 256.

def _pool_input(outer, R, inner, tag):
    g = _gen("pool", tag, outer, R, inner)
    x = torch.round(torch.randn(outer, R, inner, generator=g) * 2) / 2          # many exact ties: the first-index rule matters
    top = x.amax(dim=1, keepdim=True) + 1.0
    cols = torch.arange(inner)
    # exact ties of a new maximum: first and last row; across the first split chunk boundary (rows rpc - 1, rpc); a later pair
    x[:, 0, cols % 5 == 0] = top[:, 0, cols % 5 == 0]
    x[:, R - 1, cols % 5 <= 1] = top[:, 0, cols % 5 <= 1]
    outer_c = max(outer, 1)
    chunks = min(-(-2048 // outer_c), -(-R // 32))
    rpc = -(-R // max(chunks, 1))
    if rpc < R:
        x[:, rpc - 1, cols % 5 == 2] = top[:, 0, cols % 5 == 2] + 1
        x[:, rpc, cols % 5 == 2] = top[:, 0, cols % 5 == 2] + 1
    x[:, R // 2, cols % 5 == 3] = top[:, 0, cols % 5 == 3]
    x[:, R - 2, cols % 5 == 3] = top[:, 0, cols % 5 == 3]
    return x, torch.randn(outer, 2 * inner, generator=g)


def run_pool(outer, R, inner, op, dev):
    from svnet_amd import _ops
    x, gfull = _pool_input(outer, R, inner, op)
    xd = _leaf(x, dev)
    old, _ops.TAP = _ops.TAP, {"knn": [], "signs": [], "pools": []}
    try:
        if op == "maxmean":
            out = _ops.PoolMaxMean.apply(xd, 1)
            gout = gfull
        else:
            out = _ops.Pool.apply(xd, 1, 0 if op == "max" else 1)
            gout = gfull[:, :inner]
        arg = _ops.TAP["pools"][0].cpu().numpy() if op != "mean" else None
    finally:
        _ops.TAP = old
    out.backward(gout.to(dev))
    got = {"out0": _np(out), "dx0": _np(xd.grad)}
    x6 = x.double()
    mx, first = x6.max(dim=1).values, x6.argmax(dim=1)                          # (argmax: the first index of the maximum)
    mean = x6.mean(dim=1)
    ref_dx = torch.zeros_like(x6)
    gm = gout.double()
    if op in ("max", "maxmean"):
        ref_dx.scatter_(1, first.unsqueeze(1), gm[:, :inner].unsqueeze(1))
    if op in ("mean", "maxmean"):
        ref_dx += (gm[:, inner:] if op == "maxmean" else gm).unsqueeze(1) / R
    out6 = {"max": mx, "mean": mean, "maxmean": torch.cat([mx, mean], dim=1)}[op]
    ref = {"out0": _np(out6), "dx0": _np(ref_dx)}
    exact = ()
    if op == "max":
        exact = ("out0", "dx0")                  # values and the gradient's routing are copies
    if op == "maxmean":
        got["out_max"], ref["out_max"] = got["out0"][:, :inner], _np(mx)
        exact = ("out_max",)
    if arg is not None:
        got["arg"], ref["arg"] = arg.astype(np.int64), _np(first)
        exact = exact + ("arg",)
    return got, ref, exact


POOL_SHAPES = [(3, R, inner) for R in (255, 256, 257, 2048) for inner in (127, 128, 1022)]


@pytest.mark.parametrize("op", ["max", "mean", "maxmean"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["R%d_i%d" % (s[1], s[2]) for s in POOL_SHAPES])
def test_pool_tiers(shape, op, hip_device):
    check(*run_pool(*shape, op, hip_device), name="pool %s %r" % (op, shape))


@pytest.mark.parametrize("op", ["max", "mean"])
@pytest.mark.parametrize("shape", [(65537, 256, 1), (40, 1000, 131), (1, 4099, 3)], ids=["outer_over_65535", "wide", "one_outer"])
def test_pool_fallbacks_and_edges(shape, op, hip_device):
    """outer > 65535: the generic pool_fwd_kernel / pool_bwd_kernel even at R >= 256.  (The other fallback, outer * inner >= 2^20 at
    R >= 256, needs 2^28 elements - a GiB of float32 - and is left to the review of its one-line condition.)"""
    check(*run_pool(*shape, op, hip_device), name="pool %s %r" % (op, shape))


def run_global_pool_bn(B, N, Ca, Cb, training, act, dev):
    """GlobalMaxMeanPoolBN: bn_pool_fwd / bn_pool_bwd (BatchNorm + activation inside the split pooling pass, R = N >= 256)."""
    from svnet_amd import _ops
    g = _gen("gpbn", B, N, Ca, Cb, training, act)
    y = torch.randn(B, N, Ca, generator=g) * 2 + 0.3
    b = torch.randn(B, N, Cb, generator=g)
    gamma, beta = torch.randn(Ca, generator=g), torch.randn(Ca, generator=g) * 0.2
    rm, rv = torch.randn(Ca, generator=g) * 0.1, torch.rand(Ca, generator=g) + 0.5
    gout = torch.randn(B, 2 * (Ca + Cb), generator=g)
    yd, bd, gd, btd = (_leaf(t, dev) for t in (y, b, gamma, beta))
    rmd, rvd = rm.to(dev), rv.to(dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    out = _ops.GlobalMaxMeanPoolBN.apply(yd, bd, gd, btd, rmd, rvd, training, act, 0.2, nbt if training else None, 1e-5, 0.1)
    out.backward(gout.to(dev))
    got = {"out0": _np(out), "dx0": _np(yd.grad), "dx1": _np(bd.grad), "d:gamma": _np(gd.grad), "d:beta": _np(btd.grad),
           "buf:running_mean": _np(rmd), "buf:running_var": _np(rvd)}
    y6, b6, g6, bt6 = (t.double().requires_grad_(True) for t in (y, b, gamma, beta))
    rows = y6.reshape(-1, Ca)
    if training:
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        rm_new = 0.9 * rm.double() + 0.1 * mean.detach()
        rv_new = 0.9 * rv.double() + 0.1 * rows.detach().var(0, unbiased=True)
    else:
        mean, var, rm_new, rv_new = rm.double(), rv.double(), rm.double(), rv.double()
    z = (y6 - mean) / torch.sqrt(var + 1e-5) * g6 + bt6
    a = torch.nn.functional.leaky_relu(z, 0.2) if act == 1 else (torch.relu(z) if act == 2 else z)
    out6 = torch.cat([a.amax(1), b6.amax(1), a.mean(1), b6.mean(1)], dim=1)
    out6.backward(gout.double())
    ref = {"out0": _np(out6), "dx0": _np(y6.grad), "dx1": _np(b6.grad), "d:gamma": _np(g6.grad), "d:beta": _np(bt6.grad),
           "buf:running_mean": _np(rm_new), "buf:running_var": _np(rv_new)}
    if training:
        got["buf:nbt"], ref["buf:nbt"] = np.array([int(nbt)]), np.array([1])
    return got, ref, ()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cfg", [(4, 256, 127, 37, 1), (3, 257, 128, 21, 2), (2, 1000, 300, 64, 1)], ids=["N256", "N257", "N1000"])
def test_bn_pool_tiers(cfg, training, hip_device):
    """Continuous inputs (the activated values are fp32 results: a tie there is a rounding accident, not a rule to pin)."""
    B, N, Ca, Cb, act = cfg
    check(*run_global_pool_bn(B, N, Ca, Cb, training, act, hip_device), name="bn_pool %r" % (cfg,))


# ----------------------------------------------------------------------------- BatchNorm / VectorBN (csrc/norm.hip)
# ColMap: CW = the power of two >= C, capped at 256 (C > 256 loops over column blocks); RL = 256 / CW row lanes.  The reductions cap
# at 512 workgroups with rpb rows each: past 512 * RL * 8 rows every thread walks more than eight rows.

BN_C = [1, 3, 5, 31, 64, 65, 127, 255, 256, 257, 512, 1022]


def _bn_rows(C, big):
    cw = 1
    while cw < C and cw < 256:
        cw *= 2
    return 512 * (256 // cw) * 8 + 37 if big else 1001


def run_bnact(M, C, training, act, dev):
    from svnet_amd import _ops
    g = _gen("bnact", M, C, training, act)
    x = torch.randn(M, C, generator=g) * 1.5 + torch.randn(C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    gout = torch.randn(M, C, generator=g)
    xd, gd, bd = _leaf(x, dev), _leaf(gamma, dev), _leaf(beta, dev)
    rmd, rvd = rm.to(dev), rv.to(dev)
    nbt = torch.full((), 7, dtype=torch.int64, device=dev)
    y = _ops.BNAct.apply(xd, gd, bd, rmd, rvd, training, act, 0.2, nbt if training else None, 1e-5, 0.1)
    y.backward(gout.to(dev))
    got = {"out0": _np(y), "dx0": _np(xd.grad), "d:gamma": _np(gd.grad), "d:beta": _np(bd.grad), "buf:running_mean": _np(rmd),
           "buf:running_var": _np(rvd), "buf:nbt": np.array([int(nbt)])}
    x6, g6, b6 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    if training:
        mean, var = x6.mean(0), x6.var(0, unbiased=False)
        rm_new = 0.9 * rm.double() + 0.1 * mean.detach()
        rv_new = 0.9 * rv.double() + 0.1 * x6.detach().var(0, unbiased=True)
    else:
        mean, var, rm_new, rv_new = rm.double(), rv.double(), rm.double(), rv.double()
    z = (x6 - mean) / torch.sqrt(var + 1e-5) * g6 + b6
    y6 = torch.nn.functional.leaky_relu(z, 0.2) if act == 1 else (torch.relu(z) if act == 2 else z)
    y6.backward(gout.double())
    ref = {"out0": _np(y6), "dx0": _np(x6.grad), "d:gamma": _np(g6.grad), "d:beta": _np(b6.grad), "buf:running_mean": _np(rm_new),
           "buf:running_var": _np(rv_new), "buf:nbt": np.array([8 if training else 7])}
    return got, ref, ("buf:nbt",)


def run_vbn(M, C, training, clouds, dev):
    from svnet_amd.models.sv_layers import VectorBN
    g = _gen("vbn", M, C, training, clouds)
    v = torch.randn(clouds, M // clouds, 3, C, generator=g) * (torch.rand(C, generator=g) + 0.2)
    gate = torch.rand(clouds, C, generator=g) + 0.25 if clouds > 1 else None
    gout = torch.randn(clouds, M // clouds, 3, C, generator=g)
    bn = VectorBN(C)
    with torch.no_grad():
        bn.bn.weight.copy_(torch.randn(C, generator=g))
        bn.bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.bn.running_mean.copy_(torch.rand(C, generator=g) + 1.0)
        bn.bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bn.num_batches_tracked.fill_(3)
    rm, rv = bn.bn.running_mean.clone(), bn.bn.running_var.clone()
    gamma, beta = bn.bn.weight.detach().clone(), bn.bn.bias.detach().clone()
    bn = bn.to(dev).train(training)
    vd = _leaf(v, dev)
    gd = _leaf(gate, dev) if gate is not None else None
    out = bn(vd, gate=gd)
    out.backward(gout.to(dev))
    got = {"out0": _np(out), "dx0": _np(vd.grad), "d:gamma": _np(bn.bn.weight.grad), "d:beta": _np(bn.bn.bias.grad),
           "buf:running_mean": _np(bn.bn.running_mean), "buf:running_var": _np(bn.bn.running_var),
           "buf:nbt": np.array([int(bn.bn.num_batches_tracked)])}
    v6, g6, b6 = v.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    n = torch.linalg.vector_norm(v6, dim=-2) + 1e-6                              # [clouds, rows, C]
    rows = n.reshape(-1, C)
    if training:
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        rm_new = 0.9 * rm.double() + 0.1 * mean.detach()
        rv_new = 0.9 * rv.double() + 0.1 * rows.detach().var(0, unbiased=True)
    else:
        mean, var, rm_new, rv_new = rm.double(), rv.double(), rm.double(), rv.double()
    nb = (n - mean) / torch.sqrt(var + 1e-5) * g6 + b6
    o6 = v6 / n.unsqueeze(-2) * nb.unsqueeze(-2)
    if gate is not None:
        gt6 = gate.double().requires_grad_(True)
        o6 = o6 * gt6.view(clouds, 1, 1, C)
    o6.backward(gout.double())
    ref = {"out0": _np(o6), "dx0": _np(v6.grad), "d:gamma": _np(g6.grad), "d:beta": _np(b6.grad), "buf:running_mean": _np(rm_new),
           "buf:running_var": _np(rv_new), "buf:nbt": np.array([4 if training else 3])}
    if gate is not None:
        got["dx1"], ref["dx1"] = _np(gd.grad), _np(gt6.grad)
    return got, ref, ("buf:nbt",)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("big", [False, True], ids=["m1001", "strided"])
@pytest.mark.parametrize("C", BN_C)
def test_bnact_tiers(C, big, training, hip_device):
    act = (C % 3)                                                               # none / leaky / relu across the widths
    check(*run_bnact(_bn_rows(C, big), C, training, act, hip_device), name="bnact C=%d" % C)


VBN_CASES = [(C, clouds) for C in (1, 5, 31, 64, 65, 255, 256, 257, 512) for clouds in (1, 3)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cfg", VBN_CASES, ids=["C%d_b%d" % c for c in VBN_CASES])
def test_vbn_tiers(cfg, training, hip_device):
    C, clouds = cfg
    M = 3 * (_bn_rows(C, True) // 3 + 1)                                        # past the reductions' 512-workgroup cap, ragged
    check(*run_vbn(M, C, training, clouds, hip_device), name="vbn %r" % (cfg,))


# ----------------------------------------------------------------------------- edge gathers (csrc/gather.hip)
# diffcat_fwd_rows_kernel<NC>: row width 2 G F <= 64 / 128 / 256 / 512; diffcat_fwd_kernel beyond.  edge_xyz_edges_kernel for every
# B * N < 2^31 (edge_xyz_kernel beyond: not reachable at a testable size).

def _idx(B, N, k, g):
    idx = torch.randint(0, N, (B, N, k), generator=g)
    idx[:, ::7, :] = idx[:, ::7, :1]                                            # repeated neighbours (one point k times)
    idx[:, 1::5, 1::2] = 0                                                      # ... and one neighbour shared by many points
    idx[:, :, 0] = torch.arange(N)                                              # the point itself first, as a k-NN list has it
    return idx


def run_diffcat(B, N, k, G, F, glob, dev):
    from svnet_amd import _ops
    g = _gen("diffcat", B, N, k, G, F, glob)
    tab = torch.randn(B, N, G, F, generator=g)
    idx = _idx(B, N, k, g)
    idx_in = idx + (torch.arange(B).view(B, 1, 1) * N if glob else 0)
    gout = torch.randn(B, N, k, G, 2 * F, generator=g)
    td = _leaf(tab, dev)
    out = _ops.EdgeDiffcat.apply(td, idx_in.to(dev), bool(glob), k)
    out.backward(gout.to(dev))
    got = {"out0": _np(out), "dx0": _np(td.grad)}
    nb = tab[torch.arange(B).view(B, 1, 1), idx]                                # [B, N, k, G, F], float32: the forward is a copy
    ctr = tab.unsqueeze(2).expand(B, N, k, G, F)
    ref_out = torch.cat([nb - ctr, ctr], dim=-1)
    g6 = gout.double()
    d6 = torch.zeros(B, N, G, F, dtype=F64)
    d6.index_put_((torch.arange(B).view(B, 1, 1).expand(B, N, k), idx), g6[..., :F], accumulate=True)
    d6 += (g6[..., F:] - g6[..., :F]).sum(2)
    return got, {"out0": _np(ref_out), "dx0": _np(d6)}, ("out0",)


DIFFCAT = [(1, 32), (1, 33), (2, 32), (1, 65), (4, 32), (1, 129), (2, 128), (3, 43), (1, 257), (8, 32)]


@pytest.mark.parametrize("glob", [0, 1], ids=["local", "global"])
@pytest.mark.parametrize("gf", DIFFCAT, ids=["w%d_G%d" % (2 * g_ * f_, g_) for g_, f_ in DIFFCAT])
def test_edge_diffcat_tiers(gf, glob, hip_device):
    G, F = gf
    check(*run_diffcat(3, 203, 20, G, F, glob, hip_device), name="diffcat G=%d F=%d" % gf)


def run_edge_xyz(B, N, k, m, mode, dev):
    from svnet_amd import _ops
    g = _gen("edge_xyz", B, N, k, m, mode)
    x = torch.randn(B, 3 * m, N, generator=g)
    idx = _idx(B, N, k, g)
    out = _ops.edge_xyz(x.to(dev), idx.to(dev), mode)
    xr = x.view(B, m, 3, N).permute(0, 3, 2, 1)                                 # [B, N, 3, m] (channel = mm * 3 + d)
    nb = xr[torch.arange(B).view(B, 1, 1), idx]                                 # [B, N, k, 3, m]
    ctr = xr.unsqueeze(2).expand(B, N, k, 3, m)
    got = {"out0": _np(out)[..., :m]}
    ref = {"out0": _np(nb - ctr)}
    exact = ["out0"]
    if mode in (0, 2):
        got["out_ctr"], ref["out_ctr"] = _np(out)[..., m:2 * m], _np(ctr)
        exact.append("out_ctr")
    if mode == 1:                   # the mean over the k slots, summed in slot order in float32 as the kernel (and torch's short mean) does
        acc = torch.zeros(B, N, 3, m)
        for q in range(k):
            acc = acc + (nb[:, :, q] - xr)
        got["out_mean"], ref["out_mean"] = _np(out)[..., m:2 * m], _np((acc / k).unsqueeze(2).expand(B, N, k, 3, m))
        exact.append("out_mean")
    if mode == 2:                   # cross(x_j, x_i): a product difference (contracted to an FMA on the GPU) - against float64
        a, c = nb.double(), ctr.double()
        got["out_cross"], ref["out_cross"] = _np(out)[..., 2 * m:], _np(torch.cross(a, c, dim=3))
    return got, ref, tuple(exact)


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_edge_xyz_tiers(mode, m, hip_device):
    check(*run_edge_xyz(3, 1027, 20, m, mode, hip_device), name="edge_xyz mode=%d m=%d" % (mode, m))


# ----------------------------------------------------------------------------- loss (csrc/loss.hip smooth_ce_kernel<false>)
# One wave per row, at most 1024 workgroups of 4 waves: grid-stride past 4096 rows (part-seg: 65 536).

def run_smooth_ce(R, C, eps, dev):
    from svnet_amd import _ops
    g = _gen("ce", R, C, eps)
    logits = torch.clamp(torch.randn(R, C, generator=g) * 30, -80, 80)
    logits[::3, 0] = 80.0
    logits[1::3, C - 1] = -80.0
    target = torch.randint(0, C, (R,), generator=g)
    target[::4] = 0
    target[1::4] = C - 1
    ld = _leaf(logits, dev)
    loss = _ops.SmoothCE.apply(ld, target.to(dev), eps)
    loss.backward(torch.tensor(1.7, device=dev))
    l6 = logits.double().requires_grad_(True)
    soft = torch.full((R, C), eps / (C - 1), dtype=F64)
    soft.scatter_(1, target.view(-1, 1), 1 - eps)
    loss6 = -(soft * torch.log_softmax(l6, dim=1)).sum(1).mean()
    loss6.backward(torch.tensor(1.7, dtype=F64))
    return ({"out0": np.array([float(loss.detach())]), "dx0": _np(ld.grad)}, {"out0": np.array([float(loss6.detach())]), "dx0": _np(l6.grad)}, ())


CE_CASES = [(4097, C, eps) for C in (2, 40, 50, 64, 65, 130) for eps in (0.0, 0.2)] + \
           [(65536, 50, 0.2), (65536, 130, 0.0), (1, 40, 0.2), (7, 65, 0.2)]


@pytest.mark.parametrize("case", CE_CASES, ids=["R%d_C%d_e%g" % c for c in CE_CASES])
def test_smooth_ce_tiers(case, hip_device):
    check(*run_smooth_ce(*case, hip_device), name="smooth_ce %r" % (case,))


# ----------------------------------------------------------------------------- gate MLP (csrc/gate_mlp.h)

def run_gate(B, Cin, rows, dev):
    """rows = 0: GateMLP on pooled [B, Cin]; rows > 0: GateMLPRows on s [B, rows, Cin] (the mean inside the launch)."""
    from svnet_amd import _ops
    g = _gen("gate", B, Cin, rows)
    H, Ov = min(256, max(1, Cin // 3 + 1)), min(256, Cin // 2 + 7)
    x = torch.randn(B, rows, Cin, generator=g) if rows else torch.randn(B, Cin, generator=g)
    W0, W2 = torch.randn(H, Cin, generator=g) / Cin ** 0.5, torch.randn(Ov, H, generator=g) / H ** 0.5
    gout = torch.randn(B, Ov, generator=g)
    xd, W0d, W2d = _leaf(x, dev), _leaf(W0, dev), _leaf(W2, dev)
    if rows:
        assert _ops.GateMLPRows.supported(xd)
        gate = _ops.GateMLPRows.apply(xd, W0d, W2d)
    else:
        gate = _ops.GateMLP.apply(xd, W0d, W2d)
    gate.backward(gout.to(dev))
    x6, W06, W26 = (t.double().requires_grad_(True) for t in (x, W0, W2))
    pooled = x6.mean(1) if rows else x6
    gate6 = torch.sigmoid(torch.relu(pooled @ W06.t()) @ W26.t())
    gate6.backward(gout.double())
    return ({"out0": _np(gate), "dx0": _np(xd.grad), "d:W0": _np(W0d.grad), "d:W2": _np(W2d.grad)},
            {"out0": _np(gate6), "dx0": _np(x6.grad), "d:W0": _np(W06.grad), "d:W2": _np(W26.grad)}, ())


GATE_CASES = [(B, Cin, 0) for B in (1, 2, 32, 33) for Cin in (1, 64, 256, 257, 2048)] + \
             [(B, Cin, R) for B in (1, 2, 32, 33) for Cin, R in ((1, 1000), (64, 37), (256, 1021))]


@pytest.mark.parametrize("case", GATE_CASES, ids=["B%d_C%d_r%d" % c for c in GATE_CASES])
def test_gate_mlp_tiers(case, hip_device):
    check(*run_gate(*case, hip_device), name="gate %r" % (case,))


# ----------------------------------------------------------------------------- activations (csrc/pool.hip act kernels)

def run_act(n, kind, dev):
    from svnet_amd import _ops
    g = _gen("act", n, kind)
    x = torch.randn(n, generator=g) * 3
    x[::5] = 0.0                                                                # exact zeros: the kink's derivative follows torch's rule
    x[1::97] = -0.0
    gout = torch.randn(n, generator=g)
    xd = _leaf(x, dev)
    y = _ops.Act.apply(xd, kind)
    y.backward(gout.to(dev))
    xt = x.clone().requires_grad_(True)                                         # torch's own fp32 op: relu / leaky are exact there
    f = {1: torch.relu, 2: torch.sigmoid, 3: lambda t: torch.nn.functional.leaky_relu(t, 0.2)}[kind]
    yt = f(xt)
    yt.backward(gout)
    if kind == 2:                                                               # (expf: against float64)
        x6 = x.double().requires_grad_(True)
        y6 = torch.sigmoid(x6)
        y6.backward(gout.double())
        return {"out0": _np(y), "dx0": _np(xd.grad)}, {"out0": _np(y6), "dx0": _np(x6.grad)}, ()
    return {"out0": _np(y), "dx0": _np(xd.grad)}, {"out0": _np(yt), "dx0": _np(xt.grad)}, ("out0", "dx0")


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
@pytest.mark.parametrize("kind", [1, 2, 3], ids=["relu", "sigmoid", "leaky"])
def test_act_tiers(kind, n, hip_device):
    check(*run_act(n, kind, hip_device), name="act kind=%d n=%d" % (kind, n))


# ----------------------------------------------------------------------------- binary head (csrc/head.hip binhead_bwd_x_kernel<MP, NWV>)
# M <= 8 -> <8, 8>, <= 16 -> <16, 8>, <= 32 -> <32, 8>, > 32 -> <64, 4>: against test_hip_head.py's exact-STE oracle chain.

HEAD_M = [1, 8, 9, 16, 17, 32, 33, 64]


def run_binhead(M, dev):
    """The layer's forward and backward (dx included: binhead_bwd_x_kernel) against the oracle chain evaluated in float64 on the HIP
    run's replayed sign decisions.  The scale feeding a train-mode BatchNorm has a zero true gradient: its key carries compare_case's
    name for that (noise floor = the largest gradient of the case)."""
    from tests.test_hip_head import head_vs_oracle
    got, ref = head_vs_oracle((M, 203, 37, 1 + M % 2), dev, F64)
    for d in (got, ref):
        d["d:linear1.scale"] = d.pop("d:scale")
    return got, ref, ()


@pytest.mark.parametrize("M", HEAD_M)
def test_binhead_tiers(M, hip_device):
    check(*run_binhead(M, hip_device), name="binhead M=%d" % M)


# ----------------------------------------------------------------------------- vector tail (csrc/vtail.hip, _ops.GlobalMaxMeanPoolBNV)
# vtail_fwd_kernel<CPL> / vtail_bwd_kernel<CPL, APPLY>: C <= 64 -> 1, <= 128 -> 2, <= 192 -> 3 channels per lane; grid (chunks, B) from
# vtail_plan = split_plan(B, N, 768, 32, 8); four waves take a chunk's rows two per trip.  The cases, their inputs and the float64
# reference (the oracle's own chain) are tests/vtail_cases.py's; tests/test_host_vtail_cases.py holds the reference alone to a quarter
# of these bounds.  The HIP arg-max is replayed into the reference and certified (tests/decisions.py), not waved through.

VTAIL_REPORT = {}


def _vtail_record(name, worst_by_key, forced):
    """vtail_tier_errors.txt in the report directory of tests/test_hip_train_parity.py (OUT): worst relative error per key and case, forced arg-max decisions per case (rewritten as cases run)."""
    import os
    from tests.test_hip_train_parity import OUT
    VTAIL_REPORT[name] = (worst_by_key, forced)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vtail_tier_errors.txt"), "w") as f:
        f.write("# vector tail against float64 (tests/test_hip_kernel_tiers.py): relative error per key (tests/common.py compare_case scaling;\n"
                "# bounds %.0e for out / buf:, %.0e for gradients) and arg-max decisions forced in the replay, per case\n" % (OUT_RTOL, GRAD_RTOL))
        for n in sorted(VTAIL_REPORT):
            errs, forced_n = VTAIL_REPORT[n]
            f.write("%s  forced_argmax=%s\n" % (n, forced_n))
            for k in sorted(errs):
                f.write("    %-20s %.3e\n" % (k, errs[k]))


def vtail_hip(inp, train, dev, gate=True, binary=True, backward=True):
    """_ops.GlobalMaxMeanPoolBNV as sv_dgcnn_cls calls it -> ({key: numpy}, the recorded arg-max [B, Ca + 3C])."""
    from svnet_amd import _ops
    from tests import vtail_cases as T
    from tests.decisions import tapped
    leaves = {k: _leaf(inp[k], dev) for k in ("y", "v", "gamma1", "beta1", "gamma2", "beta2", "Wz")}
    gt = _leaf(inp["gate"], dev) if gate else None
    sc = _leaf(inp["scz"], dev) if binary else None
    stats = {k: inp[k].clone().to(dev) for k in ("rm1", "rv1", "rm2", "rv2")}
    nbt1, nbt2 = torch.full((), 3, dtype=torch.int64, device=dev), torch.full((), 5, dtype=torch.int64, device=dev)
    with tapped() as tap:
        out = _ops.GlobalMaxMeanPoolBNV.apply(leaves["y"], leaves["v"], gt, leaves["gamma1"], leaves["beta1"], stats["rm1"], stats["rv1"],
                                              leaves["gamma2"], leaves["beta2"], stats["rm2"], stats["rv2"], leaves["Wz"], sc, train, 1,
                                              T.SLOPE, nbt1 if train else None, nbt2 if train else None)
        torch.cuda.synchronize()
        assert len(tap["pools"]) == 1
        pools = tap["pools"][0].cpu().long()
    got = {"out": _np(out)}
    if backward:
        out.backward(inp["gout"].to(dev))
        torch.cuda.synchronize()
        got.update({"dy": _np(leaves["y"].grad), "dv": _np(leaves["v"].grad), "d:Wz": _np(leaves["Wz"].grad)})
        if gate:
            got["dgate"] = _np(gt.grad)
        if binary:
            got["d:scz"] = _np(sc.grad)
        for i in (1, 2):
            got["d:gamma%d" % i], got["d:beta%d" % i] = _np(leaves["gamma%d" % i].grad), _np(leaves["beta%d" % i].grad)
    for i in (1, 2):
        got["buf:running_mean%d" % i], got["buf:running_var%d" % i] = _np(stats["rm%d" % i]), _np(stats["rv%d" % i])
    got["buf:nbt"] = np.array([int(nbt1), int(nbt2)])
    return got, pools


def run_vtail(tag, train, dev, variant=None, gate=True, binary=True):
    """(got, ref, exact, info): the HIP tail and the float64 reference on the HIP run's replayed arg-max; info["dec"] certifies the replay."""
    from tests import vtail_cases as T
    inp = T.inputs(T.BY_TAG[tag], variant)
    got, pools = vtail_hip(inp, train, dev, gate, binary)
    ref, info = T.reference(inp, F64, train, pools=pools, gate=gate, binary=binary)
    ref["buf:nbt"] = np.array([4, 6] if train else [3, 5])
    info["inp"], info["pools"] = inp, pools
    return got, ref, ("buf:nbt",), info


def _vtail_errors(got, ref):
    from tests.common import case_errors
    return case_errors(got, {k: v for k, v in ref.items() if k != "buf:nbt"})


VTAIL_TAGS = ["c1_dead_lanes", "c64_last_of_1", "c65_last_of_5", "c128_last_of_12", "c129_last_of_3", "c192_widest", "one_chunk",
              "chunk_removed", "rows128"]


def test_vtail_case_list_is_the_tables():
    from tests import vtail_cases as T
    assert VTAIL_TAGS == [c[0] for c in T.CASES]


@pytest.mark.parametrize("recompute", [True, False], ids=["apply_recomputes", "apply_reads_g5"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("tag", VTAIL_TAGS)
def test_vtail_tiers(tag, train, recompute, hip_device, monkeypatch):
    """Every case of tests/vtail_cases.py, both forms of the backward's second pass (svnet_vtail_bwd_apply_f32 recomputing dL/dv5, and
    svnet_vbn_bwd_apply_f32 on the copy the first pass stores): outputs, every gradient and both norms' running statistics against float64
    on the replayed, certified arg-max; num_batches_tracked exact; a second forward on the same inputs the same bits (ordered chunk sums)."""
    from svnet_amd import config
    from tests import vtail_cases as T
    monkeypatch.setattr(config, "FUSE_VTAIL_APPLY", recompute)
    name = "%s %s %s" % (tag, "train" if train else "eval", "recompute" if recompute else "g5")
    got, ref, exact, info = run_vtail(tag, train, hip_device)
    errs = _vtail_errors(got, ref)
    print("vtail %s: %s" % (name, "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    summary = info["dec"].check()
    _vtail_record(name, errs, summary["forced"])
    assert set(ref) == set(T.KEYS) | {"buf:nbt"}
    check(got, ref, exact, "vtail " + name)
    again, pools = vtail_hip(info["inp"], train, hip_device, backward=False)
    assert np.array_equal(again["out"].view(np.uint32), got["out"].view(np.uint32)) and torch.equal(pools, info["pools"])


@pytest.mark.parametrize("form", ["no_gate", "fp_weight"])
@pytest.mark.parametrize("tag", ["c64_last_of_1", "c129_last_of_3"])
def test_vtail_optional_operands(tag, form, hip_device):
    """gate = None (no dgate: the backward's `dgate == nullptr` branch) and scz = None (fp32 Wz: the svnet_slices_sum_f32 finish)."""
    gate, binary = form != "no_gate", form != "fp_weight"
    got, ref, exact, info = run_vtail(tag, True, hip_device, gate=gate, binary=binary)
    assert ("dgate" in ref) == gate and ("d:scz" in ref) == binary and set(got) == set(ref)
    summary = info["dec"].check()
    _vtail_record("%s train %s" % (tag, form), _vtail_errors(got, ref), summary["forced"])
    check(got, ref, exact, "vtail %s %s" % (tag, form))


@pytest.mark.parametrize("recompute", [True, False], ids=["apply_recomputes", "apply_reads_g5"])
def test_vtail_zero_vectors(recompute, hip_device, monkeypatch):
    """A handful of zero vectors: the norm's gradient at 0 is 0 (torch.linalg.vector_norm; the kernel's nvv > 0 ? dn / nvv : 0), what is
    left there is g * BN(EPS) / EPS * gate, ~1e6 times an ordinary entry.  dv is compared in TWO parts, each against its own largest
    reference element - one bound over the whole tensor would leave every ordinary entry unchecked."""
    from svnet_amd import config
    from tests import vtail_cases as T
    monkeypatch.setattr(config, "FUSE_VTAIL_APPLY", recompute)
    got, ref, exact, info = run_vtail("c65_last_of_5", True, hip_device, variant="zeros")
    zero = T.zero_vectors(info["inp"]["v"]).numpy()
    assert zero.any() and np.isfinite(got["dv"]).all()
    info["dec"].check()
    errs = _vtail_errors({k: v for k, v in got.items() if k != "dv"}, {k: v for k, v in ref.items() if k != "dv"})
    (got_rest, got_zero), (ref_rest, ref_zero) = T.split_dv(got, zero), T.split_dv(ref, zero)
    errs["dv (zero vectors)"], errs["dv (the rest)"] = _vtail_errors(got_zero, ref_zero)["dv"], _vtail_errors(got_rest, ref_rest)["dv"]
    print("vtail zero vectors: |dv|max %.3e at the zero vectors, %.3e elsewhere; %s" % (
        np.abs(ref_zero["dv"]).max(), np.abs(ref_rest["dv"]).max(), "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    _vtail_record("c65_last_of_5 train zeros %s" % ("recompute" if recompute else "g5"), errs, info["dec"].check()["forced"])
    check({k: v for k, v in got.items() if k != "dv"}, {k: v for k, v in ref.items() if k != "dv"}, exact, "vtail zeros")
    check(got_zero, ref_zero, (), "vtail zeros, dv at the zero vectors")
    check(got_rest, ref_rest, (), "vtail zeros, dv elsewhere")


def test_vtail_exact_ties_take_the_first_row(hip_device):
    """One point in rows 31, 32 (either side of the first chunk boundary) and 256 (the one-row last chunk) of every cloud, scaled by 4:
    wherever the float64 maximum of a vector column is at one of the copies, the HIP arg-max is the FIRST of them - within a wave the
    strict '>', across waves and chunks the key's lower row."""
    from tests import vtail_cases as T
    tag, B, N, C, _ = T.BY_TAG["c64_last_of_1"]
    inp = T.inputs(T.BY_TAG[tag], "ties")
    got, pools = vtail_hip(inp, True, hip_device, backward=False)
    _, info = T.reference(inp, F64, True)
    own = info["f"].argmax(dim=1)[:, T.CA:]
    at_copy = sum(own == r for r in T.TIE_ROWS).bool()
    assert int(at_copy.sum()) >= 3 * C // 4
    hip = pools[:, T.CA:][at_copy]
    assert bool((hip == T.TIE_ROWS[0]).all()), "arg-max rows at the tied columns: %r" % (sorted(set(hip.tolist())),)


def test_vtail_refusals(hip_device):
    from svnet_amd import _ops, _lib
    from tests import vtail_cases as T
    assert not _ops.GlobalMaxMeanPoolBNV.supported(2, 255, 5, 64) and not _ops.GlobalMaxMeanPoolBNV.supported(2, 256, 5, 193)
    assert _ops.GlobalMaxMeanPoolBNV.supported(2, 256, 5, 192)
    inp = T.inputs(("refused", 2, 256, 193, None))
    with pytest.raises(_lib.SvnetHipError, match=r"C=193 > 192"):
        vtail_hip(inp, True, hip_device, backward=False)
    torch.cuda.synchronize()


def test_vtail_replay_has_teeth(hip_device):
    """One replayed arg-max moved to the row of its column's SMALLEST value: Decisions.check() must refuse the replay."""
    from tests import vtail_cases as T
    got, ref, exact, info = run_vtail("c65_last_of_5", True, hip_device)
    info["dec"].check()
    bad = info["pools"].clone()
    col = T.CA + 7
    bad[1, col] = int(info["f"][1, :, col].argmin())
    _, bad_info = T.reference(info["inp"], F64, True, pools=bad)
    with pytest.raises(AssertionError, match="decision replay"):
        bad_info["dec"].check()


# ----------------------------------------------------------------------------- teeth

TEETH = {
    "v2s": lambda dev: run_v2s(1001, 97, True, dev),
    "v2scat": lambda dev: run_v2scat(333, 193, False, dev),
    "vproject": lambda dev: run_vproject(333, 385, dev),
    "v2scat_sum": lambda dev: run_v2scat_sum(4, 64, 97, 300, dev),
    "pool_max": lambda dev: run_pool(3, 2048, 128, "max", dev),
    "pool_mean": lambda dev: run_pool(3, 257, 1022, "mean", dev),
    "pool_maxmean": lambda dev: run_pool(3, 256, 127, "maxmean", dev),
    "bn_pool": lambda dev: run_global_pool_bn(4, 256, 127, 37, True, 1, dev),
    "bnact": lambda dev: run_bnact(5003, 257, True, 1, dev),
    "vbn": lambda dev: run_vbn(3 * 1001, 65, True, 3, dev),
    "diffcat": lambda dev: run_diffcat(2, 64, 20, 1, 129, 0, dev),
    "edge_xyz": lambda dev: run_edge_xyz(2, 64, 20, 2, 2, dev),
    "smooth_ce": lambda dev: run_smooth_ce(4097, 65, 0.2, dev),
    "gate": lambda dev: run_gate(33, 257, 0, dev),
    "gate_rows": lambda dev: run_gate(33, 256, 1021, dev),
    "act": lambda dev: run_act(257, 2, dev),
    "binhead": lambda dev: run_binhead(33, dev),
    "vtail": lambda dev: run_vtail("c129_last_of_3", True, dev)[:3],
}


@pytest.mark.parametrize("family", sorted(TEETH) + ["pool_argmax"])
def test_each_family_check_has_teeth(family, hip_device):
    """One element of a HIP forward output off by one part in 1e4 fails the family's comparison (OUT_RTOL = 1e-5, or bit-exactness);
    for the max pool, moving one arg-max to a tied row does."""
    if family == "pool_argmax":
        got, ref, exact = run_pool(3, 2048, 128, "max", hip_device)
        check(got, ref, exact, family)
        bad = dict(got)
        bad["arg"] = got["arg"].copy()
        bad["arg"][0, 0] = 2047                 # column 0 of every outer row ties at rows 0 and R - 1: the first index is 0
        with pytest.raises(AssertionError):
            check(bad, ref, exact, "teeth:" + family)
        return
    got, ref, exact = TEETH[family](hip_device)
    teeth(got, ref, exact, family)
