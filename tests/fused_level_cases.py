"""What the tests of the three fused inference levels share (tests/test_{hip,host}_{sa_fused,fp_fused,sa_global}.py): the synthetic
layers of a level, their FoldedLevel on the device, and the comparison of results as bit patterns.  Every draw is
synth.normal(seed, 10 + 8 i + j, ...) for layer i: the arrays depend on (seed, C0, widths, kind) alone, so a file's references stay
what they were whichever test asks first."""
import numpy as np
import torch

from svnet_amd import synth
from tests import sa_fused_ref as R

F32 = np.float32


def cache():
    """A once-per-process store of references for one test file: once(key, make) -> make() the first time, the same object after."""
    ref = {}

    def once(key, make):
        if key not in ref:
            ref[key] = make()
        return ref[key]
    return once


_once = cache()


def bits(a):
    return R.positive_zero(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)


def same_bits(got, want, tag):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %r: got %r, want %r" % (
        tag, len(bad), w.size, tuple(bad[0]), g[tuple(bad[0])].view(F32), w[tuple(bad[0])].view(F32))


def dev(device, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a, order="C")).to(device) for a in arrays)      # a copy: the references are shared


def layer_state(seed, C0, widths, kind="random"):
    """Per layer the convolution and BatchNorm arrays W [w,C], b, gamma, beta, mean, var: weights ~ N(0, 1/C), BatchNorm weights of both
    signs, statistics away from identity.  kind "negative_last": the last BatchNorm has weight 0 and a negative bias - every output of
    the level is exactly 0.  "padding": the last layer has negative weights, a positive BatchNorm weight and the folded bias 8: on
    positive inputs every real row lies below 8, the value of a zero row.  "positive": positive weights and BatchNorm weights - the
    outputs grow with the inputs."""
    assert kind in ("random", "negative_last", "padding", "positive"), kind
    layers, last = [], C0
    for i, w in enumerate(widths):
        s = dict(W=(synth.normal(seed, 10 + 8 * i, (w, last)) / np.sqrt(F32(last))).astype(F32), b=synth.normal(seed, 12 + 8 * i, (w,)) * F32(0.1),
                 gamma=(synth.normal(seed, 11 + 8 * i, (w,)) + F32(0.25)).astype(F32), beta=synth.normal(seed, 13 + 8 * i, (w,)) * F32(0.2),
                 mean=synth.normal(seed, 14 + 8 * i, (w,)) * F32(0.1), var=(np.abs(synth.normal(seed, 15 + 8 * i, (w,))) + F32(0.5)).astype(F32))
        if i == len(widths) - 1:
            if kind == "negative_last":
                s["gamma"] = np.zeros_like(s["gamma"])
                s["beta"] = (-np.abs(s["beta"]) - F32(0.125)).astype(F32)
            elif kind == "padding":
                s["W"] = (-np.abs(s["W"]) * F32(0.5)).astype(F32)
                s["gamma"] = (np.abs(s["gamma"]) + F32(0.5)).astype(F32)
                s["b"], s["mean"], s["beta"] = np.zeros_like(s["b"]), np.zeros_like(s["mean"]), np.full_like(s["beta"], 8.0)
        if kind == "positive":
            s["W"], s["gamma"] = np.abs(s["W"]), (np.abs(s["gamma"]) + F32(0.5)).astype(F32)
        layers.append(s)
        last = w
    return layers


def state(seed, C0, widths, kind="random"):
    """(layer_state(...), the restatement's folded layers [(Wf, bf)] of it), made once per process."""
    def make():
        layers = layer_state(seed, C0, widths, kind)
        return layers, [R.fold(s["W"], s["b"], s["gamma"], s["beta"], s["mean"], s["var"], 1e-5) for s in layers]
    return _once((seed, C0, widths, kind), make)


def random_level(seed, C0, widths):
    """The folded layers alone: the level of the host tests."""
    return state(seed, C0, widths)[1]


def level(device, seed, C0, widths, kind="random", conv_dim=2):
    """(FoldedLevel on the device of Conv<conv_dim>d + BatchNorm<conv_dim>d layers, the restatement's folded layers); the fold's
    results are checked as bit patterns on the way."""
    from svnet_amd import sa_fused as SF
    Conv, Norm = (torch.nn.Conv1d, torch.nn.BatchNorm1d) if conv_dim == 1 else (torch.nn.Conv2d, torch.nn.BatchNorm2d)
    layers, folded = state(seed, C0, widths, kind)
    convs, bns = [], []
    for s in layers:
        conv, bn = Conv(s["W"].shape[1], s["W"].shape[0], 1), Norm(s["W"].shape[0])
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(s["W"]).reshape(conv.weight.shape))
            conv.bias.copy_(torch.from_numpy(s["b"]))
            bn.weight.copy_(torch.from_numpy(s["gamma"]))
            bn.bias.copy_(torch.from_numpy(s["beta"]))
            bn.running_mean.copy_(torch.from_numpy(s["mean"]))
            bn.running_var.copy_(torch.from_numpy(s["var"]))
        convs.append(conv.to(device))
        bns.append(bn.to(device))
    lev = SF.fold_level(convs, bns)
    for i, (Wf, bf) in enumerate(folded):
        assert np.array_equal(lev.wf[i].cpu().numpy().view(np.uint32), Wf.view(np.uint32)), "Wf of layer %d" % i
        assert np.array_equal(lev.bf[i].cpu().numpy().view(np.uint32), bf.view(np.uint32)), "bf of layer %d" % i
    return lev, folded


def fake_level(c_in, widths):
    """A FoldedLevel that was never folded, on the CPU: for the argument checks, which come before the first launch."""
    from svnet_amd import sa_fused as SF
    lev = object.__new__(SF.FoldedLevel)
    lev.c_in, lev.widths, lev.device = c_in, tuple(widths), torch.device("cpu")
    return lev
