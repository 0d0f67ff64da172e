"""GPU tests (-m gpu) of the classifier-head kernels (csrc/head.hip): the fused  act(bn(Linear(bw, ba)(x)))  over batch-size rows
against the layer-wise HIP ops (BinLinear + BNAct, pinned to the oracle by test_hip_parity.py) and against the oracle itself,
and the one-launch backward of the fp32 output layer against torch."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import sv_ref

pytestmark = pytest.mark.gpu

# (M rows, K inputs, O outputs, activation) - the two layers of the sv_dgcnn_cls / sv_pointnet_cls heads at B = 32, ragged K,
# one row word short / exactly full (M = 64), a single row group (M = 7), more than 32 rows (second half of the column words)
HEAD_SHAPES = [(32, 2044, 512, 1), (32, 512, 256, 1), (32, 1022, 512, 2), (7, 100, 24, 2), (64, 320, 40, 1), (33, 65, 9, 0),
               (16, 64, 8, 1), (1, 130, 5, 2)]


def _layer(K, O, dev, seed):
    from svnet_amd.models.sv_layers import Linear
    g = torch.Generator().manual_seed(seed)
    lin = Linear(K, O, bias=False, bw=True, ba=True)
    bn = torch.nn.BatchNorm1d(O)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(O, K, generator=g) * 0.9)              # some |W| > 1.2 (STE mask of the weights), none exactly 0 ...
        lin.weight[:, ::7] = 0.0                                           # ... except these columns: sign(0) = 0
        lin.beta.copy_(torch.randn(1, K, generator=g) * 0.3)
        lin.scale.copy_((torch.rand(1, O, generator=g) + 0.5) / K ** 0.5)
        bn.weight.copy_(torch.randn(O, generator=g))                        # negative gammas too
        bn.bias.copy_(torch.randn(O, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(O, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(O, generator=g) + 0.5)
    return lin.to(dev), bn.to(dev)


def _input(M, K, seed):
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(M, K, generator=g) * 1.1
    x = torch.round(x * 8) / 8                                              # exact zeros of x + beta are rare; exact ties are not the point here
    x[:, ::5] = 0.0
    return x


def _run(lin, bn, x, act, dev, fuse, train, gseed):
    from svnet_amd import config
    from svnet_amd.models.sv_layers import linear_bn_act
    old = config.FUSE_HEAD
    config.FUSE_HEAD = fuse
    try:
        lin.train(train), bn.train(train)
        for p in list(lin.parameters()) + list(bn.parameters()):
            p.grad = None
        xd = x.to(dev).requires_grad_(train)
        with torch.set_grad_enabled(train):
            out = linear_bn_act(lin, bn, xd, act, 0.2)
        res = {"out": out.detach().cpu().numpy().copy()}
        if train:
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(gseed)).to(dev)
            out.backward(gout)
            res["dx"] = xd.grad.cpu().numpy().copy()
            for n, p in list(lin.named_parameters()) + [("bn." + n, p) for n, p in bn.named_parameters()]:
                res["d:" + n] = p.grad.cpu().numpy().copy()
        for n, b in bn.named_buffers():
            res["buf:" + n] = b.detach().cpu().numpy().copy().astype(np.float64)
    finally:
        config.FUSE_HEAD = old
    return res


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=["%dx%dx%d_a%d" % s for s in HEAD_SHAPES])
def test_fused_head_layer_matches_layerwise(shape, train, hip_device):
    M, K, O, act = shape
    lin, bn = _layer(K, O, hip_device, 17 * M + K)
    x = _input(M, K, O)
    state = {n: b.clone() for n, b in bn.named_buffers()}
    ref = _run(lin, bn, x, act, hip_device, False, train, 5)
    for n, b in bn.named_buffers():
        b.copy_(state[n])
    got = _run(lin, bn, x, act, hip_device, True, train, 5)
    # same integer counts, same statistics (fp64 sums over <= 64 rows), same formulas: the outputs agree to rounding of the statistics
    scale = max(1.0, float(np.abs(ref["out"]).max()))
    assert np.abs(got["out"] - ref["out"]).max() <= 2e-6 * scale
    for k in ref:
        if k == "out":
            continue
        # (the scale of a linear that feeds a train-mode BatchNorm has an exactly-zero true gradient: both paths compute rounding noise
        #  there, so it is held against the largest gradient of the case - tests/common.py's rule)
        floor = 1.0 if k == "d:scale" else 1e-3
        s = max(float(np.abs(ref[k]).max()), floor * max(float(np.abs(ref[kk]).max()) for kk in ref if kk[:2] == k[:2]), 1e-30)
        err = float(np.abs(got[k] - ref[k]).max()) / s
        assert err <= (1e-4 if k == "d:scale" else 2e-5), "%s: %.3e" % (k, err)


def head_vs_oracle(shape, dev, dtype=torch.float32):
    """(got, ref): train-mode forward + backward of the fused layer and of the oracle's exact-STE restatement (sv_layers.py:35-51 +
    BatchNorm + activation) in `dtype`, with the HIP path's sign decisions replayed so that knife-edge signs cannot blur an element-wise
    comparison.  Keys: out, dx, d:weight, d:beta, d:scale, d:bn.weight, d:bn.bias."""
    from tests import decisions as D
    M, K, O, act = shape
    lin, bn = _layer(K, O, dev, 3 * M + K)
    x = _input(M, K, O)
    with D.tapped() as tap:
        got = _run(lin, bn, x, act, dev, True, True, 9)
        dec = D.decisions_of(tap)
    P = {"lin.weight": lin.weight, "lin.beta": lin.beta, "lin.scale": lin.scale, "bn.weight": bn.weight, "bn.bias": bn.bias}
    P = {n: t.detach().cpu().to(dtype).clone().requires_grad_(True) for n, t in P.items()}
    xc = x.to(dtype).clone().requires_grad_(True)
    ctx = sv_ref.Ctx(train=True, exact_ste=True)
    ctx.decisions = dec
    y = sv_ref.linear(xc, P, "lin", True, True, ctx)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + bn.eps) * P["bn.weight"] + P["bn.bias"]
    out = torch.nn.functional.leaky_relu(z, 0.2) if act == 1 else (torch.relu(z) if act == 2 else z)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(dtype)
    out.backward(gout)
    dec.check()                                                             # every replayed sign the oracle would have taken differently is a knife edge
    ref = {"out": out.detach().numpy(), "dx": xc.grad.numpy(), "d:weight": P["lin.weight"].grad.numpy(), "d:beta": P["lin.beta"].grad.numpy(),
           "d:scale": P["lin.scale"].grad.numpy(), "d:bn.weight": P["bn.weight"].grad.numpy(), "d:bn.bias": P["bn.bias"].grad.numpy()}
    return {k: got[k] for k in ref}, ref


@pytest.mark.parametrize("shape", [(32, 2044, 512, 1), (32, 512, 256, 2), (9, 200, 33, 1)], ids=["l1", "l2", "ragged"])
def test_fused_head_layer_matches_oracle(shape, hip_device):
    """Train-mode forward + backward of the fused layer against the oracle's exact-STE restatement (sv_layers.py:35-51 + BatchNorm +
    activation), with the HIP path's sign decisions replayed so that knife-edge signs cannot blur an element-wise comparison."""
    got, ref = head_vs_oracle(shape, hip_device)
    gmax = max(float(np.abs(ref[k]).max()) for k in ref if k.startswith("d:"))
    for k, r in ref.items():
        floor = gmax if k == "d:scale" else 1e-2 * gmax                     # (the scale feeding a train-mode BatchNorm has a zero true gradient)
        s = max(float(np.abs(r).max()), floor if k != "out" and k != "dx" else 0.0, 1e-30)
        err = float(np.abs(got[k] - r).max()) / s
        assert err <= 1e-3, "%s: %.3e" % (k, err)


def test_fplinear_small_backward_matches_torch(hip_device):
    from svnet_amd import _ops
    for (M, K, O) in [(32, 256, 40), (5, 33, 7), (64, 128, 50)]:
        g = torch.Generator().manual_seed(M + K)
        x, W, b, go = torch.randn(M, K, generator=g), torch.randn(O, K, generator=g), torch.randn(O, generator=g), torch.randn(M, O, generator=g)
        xd, Wd, bd = (t.to(hip_device).requires_grad_(True) for t in (x, W, b))
        _ops.FpLinear.apply(xd, Wd, bd).backward(go.to(hip_device))
        xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
        torch.nn.functional.linear(xr, Wr, br).backward(go.double())
        for got, ref in ((xd.grad, xr.grad), (Wd.grad, Wr.grad), (bd.grad, br.grad)):
            assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
