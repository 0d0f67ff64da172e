"""GPU tests (-m gpu) of the fused edge block (csrc/edgeblock.hip, edgeblock_bwd.hip, the affine weight-gradient GEMM of gemm_mfma.hip) and the
fused first layer (csrc/xyzblock.hip) over every shape they admit - not only the models' widths: every kernel instantiation of the four
launch ladders, k from 2 to 64 on both sides of the 32-edge tile, Os = 8 and 16, N = k, the XCD tile order, more than one point per wave,
and the shapes one step outside the envelope (which must run layer-wise).  tests/block_envelope_cases.py holds the cases and says which
instantiation each reaches (checked without a GPU by tests/test_host_block_envelope.py).

Every case runs the HIP path in train mode (outputs, input gradients, every parameter gradient, running statistics) and in eval mode
(outputs) against oracle.sv_ref in FLOAT64 on the HIP run's own graph - the graph itself is pinned bit for bit by the k-NN tests -
at the project's bounds: 1e-4 of the tensor's scale for outputs and running statistics, 1e-3 for gradients (tests/common.py scaling).
A spy counts the fused op: exactly one launch per forward for an admitted shape, none for a refused one.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import block_envelope_cases as T
from tests.common import case_errors
from tests.test_hip_train_parity import OUT        # the report directory of the existing block test: these reports go beside its

pytestmark = pytest.mark.gpu


def _bad(got, ref):
    """(errors, [keys beyond their bound])"""
    errs = case_errors(got, ref)
    assert set(errs) == set(ref), sorted(set(ref) - set(errs))
    tol = T.split_tolerances(errs)
    return errs, [n for n in sorted(errs, key=lambda n: -errs[n] / tol[n]) if not errs[n] <= tol[n]]


class _Spy:
    """Counts the calls of a fused autograd op (and the C entry points launched meanwhile) without changing them."""

    def __init__(self, op):
        from svnet_amd import _ops
        self.ops, self.op, self.calls, self.entries = _ops, op, 0, []

    def __enter__(self):
        self.real_apply, self.real_call = self.op.apply, self.ops.call

        def apply(*a):
            self.calls += 1
            return self.real_apply(*a)

        def call(name, *a):
            self.entries.append(name)
            return self.real_call(name, *a)
        self.op.apply, self.ops.call = apply, call
        return self

    def __exit__(self, *exc):
        del self.op.apply                       # (the override set on the subclass: autograd.Function.apply is back)
        self.ops.call = self.real_call


@functools.lru_cache(maxsize=None)
def _edge_run(tag, dev_str):
    """One edge-block case on the HIP path and on the float64 oracle: (got, ref, got_eval, ref_eval, info).  Computed once per case and
    shared by the tests that need it; nobody modifies it."""
    from svnet_amd import _ops
    from svnet_amd.models.sv_layers import SVBlock
    from svnet_amd.models.utils.sv_util import get_graph_feature_sv, svpool
    case = [c for c in T.EDGE_CASES if c[0] == tag][0]
    _, (Cs, Cv), (Os, Ov), B, N, k, expect = case
    dev = torch.device(dev_str)
    inputs = T.edge_inputs(case)
    params, s, v, rs, rv = inputs
    with T.quiet():
        blk = SVBlock((2 * Cs, 2 * Cv), (Os, Ov), binary=True)
    blk.load_state_dict(params)
    blk = blk.to(dev).train()
    sd, vd = s.to(dev).requires_grad_(True), v.to(dev).requires_grad_(True)
    with _Spy(_ops.EdgeBlock) as spy:
        edges = get_graph_feature_sv((sd, vd), k=k)
        idx = edges.idx.cpu()
        os_, ov = svpool(blk(edges))
        ((os_ * rs.to(dev)).sum() + (ov * rv.to(dev)).sum()).backward()
        torch.cuda.synchronize()
    got = {"out0": os_.detach().cpu().numpy(), "out1": ov.detach().cpu().numpy(), "dx0": sd.grad.cpu().numpy(), "dx1": vd.grad.cpu().numpy()}
    got.update({"d:" + n: p.grad.cpu().numpy() for n, p in blk.named_parameters()})
    got.update({"buf:" + n: b.detach().cpu().numpy().copy() for n, b in blk.named_buffers() if b.is_floating_point()})
    info = {"fused_train": spy.calls, "affine_wgrad": spy.entries.count("svnet_edgeblock_wgrad_f32"),
            "gemm_calls": spy.entries.count("svnet_gemm_f32")}
    # eval mode, from the same initial running statistics
    blk.load_state_dict(params)
    blk.eval()
    with _Spy(_ops.EdgeBlock) as spy, torch.no_grad():
        es, ev = svpool(blk(get_graph_feature_sv((s.to(dev), v.to(dev)), k=k)))
    info["fused_eval"] = spy.calls
    got_eval = {"out0": es.cpu().numpy(), "out1": ev.cpu().numpy()}
    # (no case needs the HIP run's decisions replayed into the oracle, as the N = 2048 block cases of test_hip_train_parity.py do: at these
    #  sizes none has a sign decision on a knife edge of rounding - tests/block_envelope_cases.py REDRAWN lists the one draw that had)
    ref = T.edge_oracle(case, inputs, idx, torch.float64, True)
    ref_eval = T.edge_oracle(case, inputs, idx, torch.float64, False)
    return got, ref, got_eval, ref_eval, info


def _report(name, payload):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, name), "w") as f:
        json.dump(payload, f, indent=0)


@pytest.mark.parametrize("case", T.EDGE_CASES, ids=[c[0] for c in T.EDGE_CASES])
def test_fused_edge_block_matches_the_float64_oracle(case, hip_device):
    tag, (Cs, Cv), (Os, Ov), B, N, k, expect = case
    got, ref, got_eval, ref_eval, info = _edge_run(tag, str(hip_device))
    errs, bad = _bad(got, ref)
    errs_eval, bad_eval = _bad(got_eval, ref_eval)
    worst = max(errs, key=lambda n: errs[n])
    print("envelope %s tiers %r: worst %.3e on %s, outputs %.3e, eval outputs %.3e" % (
        tag, expect, errs[worst], worst, max(errs["out0"], errs["out1"]), max(errs_eval.values())))
    _report("block_envelope_%s.json" % tag, {"tiers": expect, "errors": sorted(((e, n) for n, e in errs.items()), reverse=True),
                                             "eval_errors": errs_eval, "info": info})
    assert all(np.isfinite(x).all() for x in got.values())
    # a silent fall-back to the layer-wise path would make this file vacuous - and a refused shape must not reach the kernels
    want = 1 if expect is not None else 0
    assert (info["fused_train"], info["fused_eval"]) == (want, want), info
    if expect is not None:                              # the weight-gradient path svnet_edgeblock_wgrad_tier states
        assert info["affine_wgrad"] == (1 if expect["wgrad"] >= 0 else 0), info
    assert not bad, "fused edge block vs float64 oracle (%s): %r" % (tag, [(n, errs[n]) for n in bad])
    assert not bad_eval, "fused edge block, eval mode, vs float64 oracle (%s): %r" % (tag, [(n, errs_eval[n]) for n in bad_eval])


def test_a_one_percent_error_in_one_fused_gradient_is_caught(hip_device):
    """The comparison has teeth: one gradient of a new case (bwd_4_24: edgeblock_bwd_kernel<0,4,24>, never run before this file) scaled by
    1.01 must fail - on exactly that tensor.  (The parameter gradient with the largest entries: errors are measured against
    max(the tensor's own max, 1e-2 of the case's largest gradient), so 1 % of a tensor that small would be under the floor by construction.)"""
    got, ref, _, _, _ = _edge_run("bwd_4_24", str(hip_device))
    assert not _bad(got, ref)[1]
    names = [n for n in got if n.startswith("d:") and not n.endswith(".scale")]
    name = max(names, key=lambda n: float(np.abs(got[n]).max()))
    assert float(np.abs(got[name]).max()) > 2e-2 * max(float(np.abs(got[n]).max()) for n in got if n.startswith("d:")), name
    corrupted = dict(got)
    corrupted[name] = got[name] * np.float32(1.01)
    assert _bad(corrupted, ref)[1] == [name]


# ----------------------------------------------------------------------------- the fused first layer

class _FirstLayer(torch.nn.Module):
    """nc = 2: get_graph_feature -> Vector2Scalar(2,3) -> SVBlock((6,2), .) (the DGCNN callers' conv1); nc = 3: get_graph_feature_cross
    -> Vector2Scalar(3,3) -> SVBlock((9,3), .) (the PointNet callers' conv_pos)."""

    def __init__(self, out_dims, nc):
        super().__init__()
        from svnet_amd.models.sv_layers import SVBlock, Vector2Scalar
        self.nc = nc
        with T.quiet():
            self.init_scalar = Vector2Scalar(nc, 3)
            self.conv1 = SVBlock((3 * nc, nc), out_dims)

    def forward(self, x, k):
        from svnet_amd.models.utils.sv_util import get_graph_feature, get_graph_feature_cross, svpool
        v = (get_graph_feature if self.nc == 2 else get_graph_feature_cross)(x.unsqueeze(1), k=k)
        return svpool(self.conv1((self.init_scalar(v), v)))


@pytest.mark.parametrize("case", T.XYZ_CASES, ids=[c[0] for c in T.XYZ_CASES])
def test_fused_first_layer_matches_the_float64_oracle(case, hip_device):
    from svnet_amd import _ops
    tag, nc, (Os, Ov), B, N, k, tier = case
    inputs = T.xyz_inputs(case)
    params, x, rs, rv = inputs
    m = _FirstLayer((Os, Ov), nc)
    m.load_state_dict(params)
    m = m.to(hip_device).train()
    xd = x.to(hip_device)
    idx = _ops.knn(xd, k).cpu()                          # the graph the forward builds (deterministic; bit-exact with the oracle's: k-NN tests)
    with _Spy(_ops.XyzBlock) as spy:
        s, v = m(xd, k)
        ((s * rs.to(hip_device)).sum() + (v * rv.to(hip_device)).sum()).backward()
        torch.cuda.synchronize()
    fused_train = spy.calls
    got = {"out0": s.detach().cpu().numpy(), "out1": v.detach().cpu().numpy()}
    got.update({"d:" + n: p.grad.cpu().numpy() for n, p in m.named_parameters()})
    got.update({"buf:" + n: b.detach().cpu().numpy().copy() for n, b in m.named_buffers() if b.is_floating_point()})
    m.load_state_dict(params)
    m.eval()
    with _Spy(_ops.XyzBlock) as spy, torch.no_grad():
        es, ev = m(xd, k)
    got_eval = {"out0": es.cpu().numpy(), "out1": ev.cpu().numpy()}
    ref = T.xyz_oracle(case, inputs, idx, torch.float64, True)
    ref_eval = T.xyz_oracle(case, inputs, idx, torch.float64, False)
    errs, bad = _bad(got, ref)
    errs_eval, bad_eval = _bad(got_eval, ref_eval)
    worst = max(errs, key=lambda n: errs[n])
    print("envelope first layer %s tier %d: worst %.3e on %s, outputs %.3e, eval outputs %.3e" % (
        tag, tier, errs[worst], worst, max(errs["out0"], errs["out1"]), max(errs_eval.values())))
    _report("block_envelope_xyz_%s.json" % tag, {"tier": tier, "errors": sorted(((e, n) for n, e in errs.items()), reverse=True),
                                                 "eval_errors": errs_eval})
    assert all(np.isfinite(a).all() for a in got.values())
    assert (fused_train, spy.calls) == (1, 1), (fused_train, spy.calls)
    assert not bad, "fused first layer vs float64 oracle (%s): %r" % (tag, [(n, errs[n]) for n in bad])
    assert not bad_eval, "fused first layer, eval mode, vs float64 oracle (%s): %r" % (tag, [(n, errs_eval[n]) for n in bad_eval])
