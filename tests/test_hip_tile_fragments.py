"""GPU tests (-m gpu) of the weight-fragment path of the backward tile kernel (csrc/edgeblock_bwd.hip, phase B) on the smallest shapes at
which it can go wrong: three 32-edge tiles (B = 1, N = 24, k = 4), every fragment load unconditional.

A wave's three fragment slots hold the column tiles dealt to it - or the table's all-zero fragment where it has none, and for the second
k-step of Os = 8 / 16.  With Os = 128 (eight k-steps, four fragment slots refilled while the MFMAs run) the point-table widths
(8, 3), (33, 12) and (64, 24) put 5, 7 and all 10 of the column tiles in use: waves with one, two and three tiles, empty slots in
every position.  Os = 8 and 16 run one real k-step and one that reads only the zero fragment.  N = 25, k = 3 leaves the last tile ragged.

Each case runs the fused block in train mode against oracle.sv_ref in FLOAT64 on the run's own graph, with the cases' helpers and the
split tolerances of tests/block_envelope_cases.py (1e-4 outputs and running statistics, 1e-3 gradients), and checks that the fused op
and the tile kernel's instantiation were the ones meant - a silent layer-wise run would make the file vacuous.
"""
import numpy as np
import pytest
import torch

from tests import block_envelope_cases as T
from tests.common import case_errors

pytestmark = pytest.mark.gpu

# (tag, (Cs, Cv), (Os, Ov), B, N, k, tile-kernel tier 100 NKS + NC2, column tiles in use)
CASES = [
    ("frag_os128_5tiles", (8, 3), (128, 12), 1, 24, 4, 820, 5),
    ("frag_os128_7tiles", (33, 12), (128, 12), 1, 24, 4, 824, 7),
    ("frag_os128_10tiles", (64, 24), (128, 12), 1, 24, 4, 848, 10),
    ("frag_os8_padded_kstep", (8, 3), (8, 3), 1, 24, 4, 220, 5),
    ("frag_os16_zero_kstep", (8, 3), (16, 3), 1, 24, 4, 220, 5),
    ("frag_os128_ragged", (33, 12), (128, 12), 1, 25, 3, 824, 7),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tile_kernel_fragment_path_matches_the_float64_oracle(case, hip_device):
    from svnet_amd import _lib, _ops
    from svnet_amd.models.sv_layers import SVBlock
    from svnet_amd.models.utils.sv_util import get_graph_feature_sv, svpool
    tag, (Cs, Cv), (Os, Ov), B, N, k, tier, ntiles = case
    assert _lib.lib().svnet_edgeblock_bwd_tier(Cs, Cv, Os) == tier
    assert bin(T.used_tiles(Cs, Cv)).count("1") == ntiles
    assert (B * N * k % 32 != 0) == tag.endswith("ragged")
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
    print("tile fragments %s (tier %d, %d column tiles): worst %.3e of %.0e on %s" % (tag, tier, ntiles, errs[worst], tol[worst], worst))
    assert all(np.isfinite(x).all() for x in got.values())
    bad = [(n, errs[n]) for n in sorted(errs, key=lambda n: -errs[n] / tol[n]) if not errs[n] <= tol[n]]
    assert not bad, "fused edge block vs float64 oracle (%s): %r" % (tag, bad)
