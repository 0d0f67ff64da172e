"""GPU tests (-m gpu) of the forward edge kernels (csrc/edgeblock.hip) on the smallest shapes at which their lane masks, the SAVE split and
the 32-bit neighbour rows can go wrong: B = 2, N = 24 (two clouds, so a row offset carries a cloud's first point), every case about a second.

The kernels ballot a raw comparison and AND it with a wave-uniform lane mask (wave.h wave_ballot_masked) taken as the ballot of `lane < Cs`
and `lane < 2 Cv`: the widths 1, 31, 32, 33, 63 and 64 put the mask's edge at the first bit, on both sides of the half-word and at the full
word (where a shifted mask would be undefined), in the one-edge kernels <OP, NARROW> and in the two-edge kernel, whose predicate repeats per
half-wave.  Train mode runs the SAVE instantiation (n16 and the planes kept: outputs, input gradients, parameter gradients and running
statistics are checked), eval mode under no_grad the other one (outputs).  An odd k runs the edge behind the unrolled pair, k = 2 the
loop with no tail.

No k = 1 case: the fused path does not admit it (sv_layers.edge_block_shape_ok asks 2 <= k, and svnet_edgeblock_wgrad_tier refuses every
k < 8 while svnet_edgeblock_fwd_tier / svnet_edgeblock_bwd_tier do not look at k), so a k = 1 layer runs layer-wise and never reaches
these kernels (tests/test_host_edge_forward_rows.py asks them).

Each case runs the fused block against oracle.sv_ref in FLOAT64 on the run's own graph, with the helpers and the split tolerances of
tests/block_envelope_cases.py (1e-4 outputs and running statistics, 1e-3 gradients), asserts the forward tier first, and checks through a
spy on _ops.call that svnet_edgeblock_fwd_f32 ran exactly once per forward - a silent layer-wise run would make the file vacuous.
"""
import numpy as np
import pytest
import torch

from tests import block_envelope_cases as T
from tests.common import case_errors

pytestmark = pytest.mark.gpu

B, N = 2, 24
# (tag, (Cs, Cv), (Os, Ov), k, forward tier)
CASES = [
    ("two_1_1_k3", (1, 1), (8, 1), 3, T.TWO),
    ("two_31_15_k2", (31, 15), (32, 32), 2, T.TWO),
    ("two_32_16_k3", (32, 16), (32, 32), 3, T.TWO),
    ("t111_32_1_k3", (32, 1), (64, 8), 3, 111),
    ("t111_31_16_k2", (31, 16), (64, 33), 2, 111),
    ("t110_33_1_k3", (33, 1), (64, 8), 3, 110),
    ("t110_63_31_k2", (63, 31), (64, 64), 2, 110),
    ("t110_64_32_k5", (64, 32), (64, 64), 5, 110),
    ("t121_1_16_k3", (1, 16), (128, 12), 3, 121),
    ("t121_32_16_k2", (32, 16), (128, 42), 2, 121),
    ("t120_33_17_k3", (33, 17), (128, 42), 3, 120),
    ("t120_63_32_k2", (63, 32), (128, 64), 2, 120),
    ("t120_64_32_k5", (64, 32), (128, 64), 5, 120),
]
# Draws that put a sign decision on a knife edge of rounding are drawn again under another stream name, never given a looser bound
# (tests/block_envelope_cases.py REDRAWN does the same for its table): {tag: draw}.  None was needed.
REDRAWN = {}


def _ecase(case):
    tag, cin, cout, k, _ = case
    return ("fwd_masks/%s" % tag + ("#%d" % REDRAWN[tag] if tag in REDRAWN else ""), cin, cout, B, N, k, None)


def _run(tag, dev_str):
    """One case on the HIP path (train, then eval) and on the float64 oracle: (got, ref, got_eval, ref_eval, launches)."""
    from svnet_amd import _ops
    from svnet_amd.models.sv_layers import SVBlock
    from svnet_amd.models.utils.sv_util import get_graph_feature_sv, svpool
    case = [c for c in CASES if c[0] == tag][0]
    _, (Cs, Cv), (Os, Ov), k, _ = case
    ecase = _ecase(case)
    dev = torch.device(dev_str)
    inputs = T.edge_inputs(ecase)
    params, s, v, rs, rv = inputs
    with T.quiet():
        blk = SVBlock((2 * Cs, 2 * Cv), (Os, Ov), binary=True)
    blk.load_state_dict(params)
    blk = blk.to(dev).train()
    sd, vd = s.to(dev).requires_grad_(True), v.to(dev).requires_grad_(True)
    entries, real_call = [], _ops.call

    def call(name, *a):
        entries.append(name)
        return real_call(name, *a)
    _ops.call = call
    try:
        edges = get_graph_feature_sv((sd, vd), k=k)
        idx = edges.idx.cpu()
        os_, ov = svpool(blk(edges))
        launches = {"train": entries.count("svnet_edgeblock_fwd_f32")}
        ((os_ * rs.to(dev)).sum() + (ov * rv.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        got = {"out0": os_.detach().cpu().numpy(), "out1": ov.detach().cpu().numpy(), "dx0": sd.grad.cpu().numpy(), "dx1": vd.grad.cpu().numpy()}
        got.update({"d:" + n: p.grad.cpu().numpy() for n, p in blk.named_parameters()})
        got.update({"buf:" + n: b.detach().cpu().numpy().copy() for n, b in blk.named_buffers() if b.is_floating_point()})
        # eval mode, from the same initial running statistics: nothing is kept for a backward
        blk.load_state_dict(params)
        blk.eval()
        del entries[:]
        with torch.no_grad():
            es, ev = svpool(blk(get_graph_feature_sv((s.to(dev), v.to(dev)), k=k)))
            torch.cuda.synchronize()
        launches["eval"] = entries.count("svnet_edgeblock_fwd_f32")
    finally:
        _ops.call = real_call
    got_eval = {"out0": es.cpu().numpy(), "out1": ev.cpu().numpy()}
    ref = T.edge_oracle(ecase, inputs, idx, torch.float64, True)
    ref_eval = T.edge_oracle(ecase, inputs, idx, torch.float64, False)
    return got, ref, got_eval, ref_eval, launches


def _bad(got, ref):
    errs = case_errors(got, ref)
    # every key of the oracle is compared (Ov = 1 leaves the gate MLP a hidden layer of width 0: case_errors passes over its empty weights)
    assert set(errs) == {n for n in ref if ref[n].size}, sorted(set(ref) - set(errs))
    tol = T.split_tolerances(errs)
    return errs, tol, [(n, errs[n]) for n in sorted(errs, key=lambda n: -errs[n] / tol[n]) if not errs[n] <= tol[n]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_kernel_matches_the_float64_oracle_in_train_and_eval_mode(case, hip_device):
    from svnet_amd import _lib
    from svnet_amd.models.sv_layers import edge_block_shape_ok
    tag, (Cs, Cv), (Os, Ov), k, tier = case
    assert _lib.lib().svnet_edgeblock_fwd_tier(Cs, Cv, Os, Ov, B, N) == tier
    assert edge_block_shape_ok(Cs, Cv, Os, Ov, k, N)
    got, ref, got_eval, ref_eval, launches = _run(tag, str(hip_device))
    errs, tol, bad = _bad(got, ref)
    errs_eval, _, bad_eval = _bad(got_eval, ref_eval)
    worst = max(errs, key=lambda n: errs[n] / tol[n])
    print("forward masks %s (tier %d): worst %.3e of %.0e on %s, eval outputs %.3e" % (tag, tier, errs[worst], tol[worst], worst, max(errs_eval.values())))
    assert launches == {"train": 1, "eval": 1}, launches
    assert all(np.isfinite(x).all() for x in got.values()) and all(np.isfinite(x).all() for x in got_eval.values())
    assert not bad, "fused edge block, train mode, vs float64 oracle (%s): %r" % (tag, bad)
    assert not bad_eval, "fused edge block, eval mode, vs float64 oracle (%s): %r" % (tag, bad_eval)

