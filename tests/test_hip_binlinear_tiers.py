"""GPU tests (-m gpu): every dispatch tier of the binarized dense layer's kernels against the numpy restatement tests/binlinear_ref.py.

The case tables are tests/binlinear_cases.py (stated once; tests/test_host_binlinear_cases.py checks the tables, the restatement and the
comparators on the CPU).  Every case calls the C interface directly, after asserting that svnet_binlinear_tier /
svnet_binlinear_i8_tier name the tier the case is meant for.  The popcount kernel gets the REFERENCE's weight planes, so its cases do
not lean on svnet_binweight_prepare_f32 (which has cases of its own).  Outputs are pre-filled with sentinels and compared whole: y's
trailing rows and each plane's extra 64-row block must keep them.  exact cases are compared bit for bit, real cases per element with the
derived bounds of binlinear_cases.py.  The five cases beyond 131072 rows build their inputs and their reference on the device (a float64
product of the ternary operands: exact, and independent of the code under test)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import binlinear_cases as B
from tests import binlinear_ref as R

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dev):
    if a is None:
        return None
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _assert_popcount_plan(c):
    for chunk in range(len(c["chunks"])):
        rc, got = B.plan_of(c, chunk)
        want = B.expected_plan(c, chunk)
        assert rc == 0 and got == want, "%s chunk %d: %r" % (c["name"], chunk, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


def _report(c, kind, r, y):
    if kind == "real" and y.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.nan_to_num(np.abs(y.astype(np.float64) - r["y"]) / (B.EPS24 * (r["mag"] + np.abs(r["y"]))), nan=0.0)
        print("%s real: worst element %.3f of its bound" % (c["name"], q.max()))


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", B.POPCOUNT_HOST, ids=[c["name"] for c in B.POPCOUNT_HOST])
def test_popcount_case(c, kind, hip_device):
    from svnet_amd import _lib
    _assert_popcount_plan(c)
    M, K, O = c["M"], c["K"], c["O"]
    d = B.build_forward(c, kind)
    r = B.reference_forward(c, d)
    ws, wz, _, _ = R.weight_prepare(d.W)
    t = {n: _dev(a, hip_device) for n, a in (("x", d.x_store), ("beta", d.beta), ("ws", ws), ("wz", wz), ("scale", d.scale), ("bias", d.bias))}
    y = _dev(B.y_storage(c), hip_device)
    planes = [_dev(B.plane_storage(c), hip_device) for _ in range(3)] if c["planes"] else [None] * 3
    _lib.call("svnet_binlinear_fwd_f32", _p(t["x"]), d.ldx, _p(t["beta"]), _p(t["ws"]), _p(t["wz"]), _p(t["scale"]), _p(t["bias"]), M, K, O,
              _p(y), _p(planes[0]), _p(planes[1]), _p(planes[2]), _stream())
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    _report(c, kind, r, yh[:M])
    bad = B.y_failures(c, kind, r, yh)
    if c["planes"]:
        bad += B.plane_failures(c, r, dict(zip(("x_sign", "x_nz", "x_ste"), map(_words, planes))))
    assert not bad, "\n".join(bad)


def _plant_on_device(x, beta, W):
    """The planted values of binlinear_cases.build_forward, by strides (the large cases are built on the device)."""
    up = torch.nextafter(torch.tensor(1.2, device=x.device), torch.tensor(2.0, device=x.device))
    beta[::4] = 0.0
    beta[1::8] = -0.0
    xf, wf = x.view(-1), W.view(-1)
    xf[::17] = 0.0
    xf[5::29] = -0.0
    x[2::23] = -beta                                                               # whole rows with t == 0
    x[1::19, ::4], x[4::19, ::4], x[7::19, ::4], x[10::19, ::4] = 1.2, -1.2, up, -up   # (columns with beta == 0)
    wf[::11] = 0.0
    wf[3::37] = -0.0
    wf[1::41], wf[2::43] = 1.2, -1.2


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", B.POPCOUNT_DEVICE, ids=[c["name"] for c in B.POPCOUNT_DEVICE])
def test_popcount_case_beyond_131072_rows(c, kind, hip_device):
    from svnet_amd import _lib
    _assert_popcount_plan(c)
    M, K, O = c["M"], c["K"], c["O"]
    dev = hip_device
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(("%s/%s" % (c["name"], kind)).encode()))
    x, beta, W = (torch.randn(s, generator=g, device=dev) for s in ((M, K), (K,), (O, K)))
    _plant_on_device(x, beta, W)
    d = B.Data()
    rng = np.random.default_rng(int(g.initial_seed()))
    d.scale, d.bias = B.scale_bias(rng, O, kind, c["bias"])
    sc, bs = _dev(d.scale, dev), _dev(d.bias, dev)
    ws, wz, _, _ = R.weight_prepare(W.cpu().numpy())
    ws, wz = _dev(ws, dev), _dev(wz, dev)
    y = torch.full((M + B.Y_GUARD_ROWS, O), B.Y_SENTINEL, device=dev)
    _lib.call("svnet_binlinear_fwd_f32", _p(x), K, _p(beta), _p(ws), _p(wz), _p(sc), _p(bs), M, K, O, _p(y), None, None, None, _stream())
    # the reference: one float32 add, signs, a float64 product of ternary operands (every partial sum an exact integer), float64 epilogue
    t = x + beta
    assert bool((t == 0).any()) and bool((t == 1.2).any()) and bool((t == -1.2).any())
    cnt = torch.sign(t).double() @ torch.sign(W).double().t()
    assert bool((cnt == cnt.round()).all()) and float(cnt.abs().max()) <= K
    prod = cnt * sc.double()
    ref = prod + bs.double()
    got = y[:M].double()
    assert bool((y[M:] == B.Y_SENTINEL).all()), "%s: rows past M were written" % c["name"]
    if kind == "exact":
        assert bool((ref.float().double() == ref).all())
        nbad = int((got != ref).sum())
        assert nbad == 0, "%s [exact]: %d of %d elements differ" % (c["name"], nbad, got.numel())
    else:
        err, bound = (got - ref).abs(), B.EPS24 * (prod.abs() + ref.abs())
        print("%s real: worst element %.3f of its bound" % (c["name"], float((err / bound.clamp_min(1e-300)).max())))
        nbad = int((~(err <= bound)).sum())
        assert nbad == 0, "%s [real]: %d of %d elements out of bound" % (c["name"], nbad, got.numel())


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", B.I8, ids=[c["name"] for c in B.I8])
def test_i8_case(c, kind, hip_device):
    from svnet_amd import _lib
    L = _lib.lib()
    rc, got = B.i8_plan_of(c)
    assert rc == 0 and got == B.expected_i8_plan(c), (c["name"], got)
    M, K, O = c["M"], c["K"], c["O"]
    d = B.build_forward(c, kind)
    r = B.reference_forward(c, d)
    t = {n: _dev(a, hip_device) for n, a in (("x", d.x_store), ("beta", d.beta), ("W", d.W), ("scale", d.scale), ("bias", d.bias),
                                             ("cloud_n", d.cloud_n))}
    nbytes = L.svnet_binweight_i8_bytes(O, K)
    assert nbytes == O * 128 * c["nchunks"]
    w8 = torch.full((nbytes + 16,), 0x55, dtype=torch.int8, device=hip_device)
    _lib.call("svnet_binweight_pack_i8", _p(t["W"]), O, K, _p(w8), _stream())
    y = _dev(B.y_storage(c), hip_device)
    planes = [_dev(B.plane_storage(c), hip_device) for _ in range(3)] if c["planes"] else [None] * 3
    sums = torch.zeros(B.sliced_len(2 * O), dtype=torch.float64, device=hip_device) if c["sums"] else None
    args = (_p(t["x"]), d.ldx, _p(t["beta"]), _p(w8), _p(t["scale"]), _p(t["bias"]), M, K, O, _p(y), _p(planes[0]), _p(planes[1]), _p(planes[2]),
            _p(sums))
    if c["cloud"]:
        _lib.call("svnet_binlinear_i8_cloud_fwd_f32", *args, _p(t["cloud_n"]), c["cloud"], _stream())
    else:
        _lib.call("svnet_binlinear_i8_fwd_f32", *args, _stream())
    if sums is not None:
        _lib.call("svnet_slices_sum_f64", _p(sums), 2 * O, _stream())
    torch.cuda.synchronize()
    assert bool((w8[nbytes:] == 0x55).all()), "%s: svnet_binweight_pack_i8 wrote past its buffer" % c["name"]
    yh = y.cpu().numpy()
    _report(c, kind, r, yh[:M])
    bad = B.y_failures(c, kind, r, yh)
    if c["planes"]:
        bad += B.plane_failures(c, r, dict(zip(("x_sign", "x_nz", "x_ste"), map(_words, planes))))
    if sums is not None:
        bad += B.colsum_failures(c, r, d, sums[:2 * O].cpu().numpy())
        assert bool((sums[-2:] == 0).all()), "%s: the accumulator's two spare elements were written" % c["name"]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", B.PREPARE, ids=[c["name"] for c in B.PREPARE])
def test_binweight_prepare_case(c, kind, hip_device):
    from svnet_amd import _lib
    O, K = c["O"], c["K"]
    KW = (K + 63) // 64
    rng = B._rng(c, kind)
    W = B.plant_weights(rng, rng.standard_normal(size=(O, K), dtype=np.float32))
    scale, _ = B.scale_bias(rng, O, kind)
    ws, wz, wb, weff = R.weight_prepare(W, scale)
    dev = hip_device
    guard_f, guard_w = np.float32(B.Y_SENTINEL), B.PLANE_SENTINEL
    o_ws, o_wz = (_dev(np.full(O * KW + 1, guard_w, np.uint64), dev) for _ in range(2))
    o_wb, o_we = (_dev(np.full(O * K + 1, guard_f, np.float32), dev) for _ in range(2))
    mode = c["mode"]
    Wd, sd = _dev(W, dev), _dev(scale, dev)                                        # (named: the call gets bare addresses)
    _lib.call("svnet_binweight_prepare_f32", _p(Wd), _p(sd) if mode == "all" else None, O, K, _p(o_ws), _p(o_wz),
              _p(o_wb) if mode != "planes" else None, _p(o_we) if mode == "all" else None, _stream())
    torch.cuda.synchronize()
    for name, got, ref, guard in (("w_sign", _words(o_ws), ws.reshape(-1), guard_w), ("w_nz", _words(o_wz), wz.reshape(-1), guard_w),
                                  ("w_b", o_wb.cpu().numpy(), wb.reshape(-1) if mode != "planes" else None, guard_f),
                                  ("w_eff", o_we.cpu().numpy(), weff.reshape(-1) if mode == "all" else None, guard_f)):
        assert got[-1] == guard, "%s: %s written past its end" % (c["name"], name)
        if ref is None:
            assert np.all(got == guard), "%s: %s written though not asked for" % (c["name"], name)
        else:
            assert np.array_equal(got[:-1], ref), "%s: %s differs" % (c["name"], name)       # (values: w_b's -0 would equal +0; sign() gives neither)
            if got.dtype == np.float32:
                assert not np.signbit(got[:-1][ref == 0]).any()


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("c", B.GRAD, ids=[c["name"] for c in B.GRAD])
def test_binweight_grad_case(c, kind, hip_device):
    from svnet_amd import _lib
    O, K = c["O"], c["K"]
    d = B.build_grad(c, kind)
    dev = hip_device
    guard = np.float32(B.Y_SENTINEL)
    dW0 = np.concatenate([(d.dW0 if c["accumulate"] else np.full((O, K), guard, np.float32)).reshape(-1), [guard]]).astype(np.float32)
    ds0 = np.concatenate([d.dscale0 if c["accumulate"] else np.full(O, guard, np.float32), [guard]]).astype(np.float32)
    dW, ds = (None if c["eval"] else _dev(dW0, dev)), _dev(ds0, dev)
    sb = _dev(d.sum_store, dev)
    GX, W, sc = _dev(d.GX_store, dev), _dev(d.W, dev), _dev(d.scale, dev)          # (named: the call gets bare addresses)
    _lib.call("svnet_binweight_grad_f32", _p(GX), _p(W), _p(sc), O, K, _p(dW), _p(ds),
              c["accumulate"], c["gx_sliced"], _p(sb), c["sum_len"], _stream())
    torch.cuda.synchronize()
    dsh = ds.cpu().numpy()
    assert dsh[-1] == guard and (dW is None or dW.cpu().numpy()[-1] == guard), "%s: written past the end" % c["name"]
    bad = B.grad_failures(c, d, None if dW is None else dW.cpu().numpy()[:-1].reshape(O, K), dsh[:-1], None if sb is None else sb.cpu().numpy())
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M,K,O,family", [(1023, 70, 64, "popcount"), (1024, 70, 63, "popcount"), (1024, 70, 64, "i8")],
                         ids=["1023x70x64", "1024x70x63", "1024x70x64"])
def test_python_gate_on_both_sides_of_both_edges(M, K, O, family, hip_device):
    """_ops.BinLinear sends M >= 1024 and O >= 64 to the matrix cores: train mode, forward and backward against the oracle on either
    side of either edge, with the kernel family that ran read off the binding's call record and its tier off the queries."""
    from oracle import sv_ref
    from svnet_amd import _lib, config
    from svnet_amd.models.sv_layers import Linear
    from tests.common import compare_case
    from tests.golden import cases as C
    from tests.golden import harness as H
    from tests.test_hip_parity import RTOL
    assert config.BINLINEAR_MFMA
    params = H.module_params("Linear", (K, O, False, True, True), "gate%dx%d" % (M, O))
    x = C.t("gate_lin/%dx%d" % (M, O), (M, K), 1.0)
    x.view(-1)[::11] = 0.0
    params["beta"][:, ::5] = 0.0
    r = C.t("gate_lin_r/%dx%d" % (M, O), (M, O))
    m = Linear(K, O, False, bw=True, ba=True)
    m.load_state_dict(params)
    m = m.to(hip_device).train()
    xd = x.to(hip_device).requires_grad_(True)
    timers = {n: _lib.KernelTimer(n) for n in ("svnet_binlinear_fwd_f32", "svnet_binlinear_i8_fwd_f32")}
    _lib.TIMERS.extend(timers.values())
    try:
        y = m(xd)
    finally:
        for t in timers.values():
            _lib.TIMERS.remove(t)
    ran = {n: len(t.pairs) for n, t in timers.items()}
    assert ran == {"svnet_binlinear_fwd_f32": int(family == "popcount"), "svnet_binlinear_i8_fwd_f32": int(family == "i8")}, ran
    if family == "i8":
        rc, plan = B.i8_plan_of(dict(M=M, K=K, O=O, sums=1))
        assert rc == 0 and (plan["ntw"], plan["grid_x"], plan["grid_y"], plan["nchunks"]) == (1, 8, 1, 1)
    else:
        rc, plan = B.plan_of(dict(M=M, K=K, O=O), 0)
        assert rc == 0 and (plan["nchunk"], plan["kwm"], plan["ppm"], plan["form"], plan["og_shift"], plan["grid_tiles"]) == (1, 2, 1, B.LOOP, 6, 16)
    (y * r.to(hip_device)).sum().backward()
    P = {"m." + k: v.clone().requires_grad_(True) for k, v in params.items()}
    xo = x.clone().requires_grad_(True)
    yo = sv_ref.linear(xo, P, "m", bw=True, ba=True, ctx=sv_ref.Ctx(train=True))
    (yo * r).sum().backward()
    got = {"out0": y.detach().cpu().numpy(), "dx0": xd.grad.cpu().numpy(), "d:weight": m.weight.grad.cpu().numpy(),
           "d:beta": m.beta.grad.cpu().numpy(), "d:scale": m.scale.grad.cpu().numpy()}
    ref = {"out0": yo.detach().numpy(), "dx0": xo.grad.numpy(), "d:weight": P["m.weight"].grad.numpy(),
           "d:beta": P["m.beta"].grad.numpy(), "d:scale": P["m.scale"].grad.numpy()}
    compare_case(got, ref, RTOL, "binlinear gate %dx%dx%d" % (M, K, O))
