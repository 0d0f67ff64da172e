"""GPU tests (-m gpu) of the row passes of the backward tile kernel (csrc/edgeblock_bwd.hip, phase C in its eight-rows-per-wave form) on
the smallest shapes at which they can go wrong: a handful of 32-edge tiles per case.

A wave owns eight consecutive edge rows.  Passes 1 and 4 walk them straight-line on row positions derived once: the point of every row,
the row behind which a point's centre sums go out, and which of the two early-requested sets of per-cloud constants a row takes.  Rows past
E repeat the wave's last row.  The cases put

  point boundaries  inside a wave's rows: k = 2 (four points per wave), k = 3 (uneven), k = 9 (one change, at another row in every wave),
                    k = 20 (the models' own), with N = 24 or 25 so that k <= N;
  a cloud boundary  inside a wave's rows and between the waves of a tile: B = 3, N = 25, k = 3 has 75 edge rows per cloud, so the second
                    cloud starts in row 3 of wave 1 of tile 2 and the third in row 6 of wave 2 of tile 4; its E = 225 also leaves a last
                    tile with ONE row (waves 1 - 3 without a row);
  ragged ends       E mod 32 = 1, 9 (N = 25, k = 17: wave 1 has one row) and 31 (N = 25, k = 23: wave 3 misses its last row);
  a third cloud     under one wave: B = 8, N = 3, k = 2 has six edge rows per cloud - the branch that takes the constants from the table

on the five forms of the phase (tile-kernel tier 100 NKS + NC2), with the point-table widths tests/test_hip_tile_fragments.py and
tests/block_envelope_cases.py use for these tiers.  Tiers 420 and 844 (conv2 / conv3 and conv4 of the models) get every pattern.

Each case runs the fused block in train mode against oracle.sv_ref in FLOAT64 on the run's own graph, with the helpers and the split
tolerances of tests/block_envelope_cases.py (1e-4 outputs and running statistics, 1e-3 gradients), and checks that the fused op and the
tile kernel's instantiation were the ones meant.
"""
import numpy as np
import pytest
import torch

from tests import block_envelope_cases as T
from tests.common import case_errors

pytestmark = pytest.mark.gpu

# point-table widths (Cs, Cv) -> (Os, Ov) of the five forms, by tier
FORMS = {
    220: ((8, 3), (8, 3)),
    420: ((32, 10), (64, 21)),          # conv3
    844: ((64, 21), (128, 42)),         # conv4
    824: ((33, 12), (128, 12)),
    848: ((64, 24), (128, 12)),         # a neighbour row in two loads (lane and lane + 64)
}
# (pattern, B, N, k, E mod 32)
CLOUD = ("cloud_k3_rag1", 3, 25, 3, 1)
K2 = ("k2", 1, 24, 2, 16)
K9 = ("k9_rag1", 1, 25, 9, 1)
K20 = ("k20", 1, 25, 20, 20)
RAG9 = ("k17_rag9", 1, 25, 17, 9)
RAG31 = ("k23_rag31", 1, 25, 23, 31)
THIRD = ("third_cloud", 8, 3, 2, 16)
PLAN = [
    (420, (CLOUD, K2, K9, K20, RAG9, RAG31)),
    (844, (CLOUD, K2, K9, K20, RAG9, RAG31)),
    (220, (CLOUD, RAG31, THIRD)),
    (824, (CLOUD, RAG9)),
    (848, (CLOUD, RAG31)),
]
CASES = [("rows_t%d_%s" % (tier, pat[0]),) + FORMS[tier] + pat[1:4] + (tier, pat[4]) for tier, pats in PLAN for pat in pats]
assert all(c[3] * c[4] * c[5] <= T.MAX_EDGES // 10 and c[5] <= c[4] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tile_kernel_row_passes_match_the_float64_oracle(case, hip_device):
    from svnet_amd import _lib, _ops
    from svnet_amd.models.sv_layers import SVBlock
    from svnet_amd.models.utils.sv_util import get_graph_feature_sv, svpool
    tag, (Cs, Cv), (Os, Ov), B, N, k, tier, rag = case
    assert _lib.lib().svnet_edgeblock_bwd_tier(Cs, Cv, Os) == tier
    assert B * N * k % 32 == rag
    ecase = case[:6] + (None,)
    inputs = T.edge_inputs(ecase)
    params, s, v, rs, rv = inputs
    with T.quiet():
        blk = SVBlock((2 * Cs, 2 * Cv), (Os, Ov), binary=True)
    blk.load_state_dict(params)
    blk = blk.to(hip_device).train()
    sd, vd = s.to(hip_device).requires_grad_(True), v.to(hip_device).requires_grad_(True)
    entries, real_call = [], _ops.call

    def call(name, *a):
        entries.append(name)
        return real_call(name, *a)
    _ops.call = call
    try:
        edges = get_graph_feature_sv((sd, vd), k=k)
        idx = edges.idx.cpu()
        os_, ov = svpool(blk(edges))
        ((os_ * rs.to(hip_device)).sum() + (ov * rv.to(hip_device)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        _ops.call = real_call
    assert entries.count("svnet_edgeblock_bwd_f32") >= 1, entries          # the fused backward ran (its two parts may be two launches)
    got = {"out0": os_.detach().cpu().numpy(), "out1": ov.detach().cpu().numpy(), "dx0": sd.grad.cpu().numpy(), "dx1": vd.grad.cpu().numpy()}
    got.update({"d:" + n: p.grad.cpu().numpy() for n, p in blk.named_parameters()})
    got.update({"buf:" + n: b.detach().cpu().numpy().copy() for n, b in blk.named_buffers() if b.is_floating_point()})
    ref = T.edge_oracle(ecase, inputs, idx, torch.float64, True)
    errs = case_errors(got, ref)
    assert set(errs) == set(ref), sorted(set(ref) - set(errs))
    tol = T.split_tolerances(errs)
    worst = max(errs, key=lambda n: errs[n] / tol[n])
    print("tile row passes %s (tier %d, E = %d): worst %.3e of %.0e on %s" % (tag, tier, B * N * k, errs[worst], tol[worst], worst))
    assert all(np.isfinite(x).all() for x in got.values())
    bad = [(n, errs[n]) for n in sorted(errs, key=lambda n: -errs[n] / tol[n]) if not errs[n] <= tol[n]]
    assert not bad, "fused edge block vs float64 oracle (%s): %r" % (tag, bad)
