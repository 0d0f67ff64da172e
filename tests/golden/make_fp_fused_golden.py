#!/usr/bin/env python3
"""Generate tests/golden/fp_fused.npz: the REFERENCE's feature-propagation level in eval mode on small lattice inputs, recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_fp_fused_golden          (from the repo root, CPU)

For every case of tests/fp_fused_ref.GOLDEN_CASES -
    a    B 2, N 96, S 24, D1 5, D2 7, widths (12, 16)
    s1   B 2, N 16, S 1, D1 0 (points1 = None), D2 6, widths (8,): the reference's `S == 1` branch
- it runs `PointNetFeaturePropagation(D1 + D2, mlp)` of the reference's models/utils/pointnet_util.py in eval mode and stores data
only, no reference source, under "<name>_...":
  - the inputs "xyz1" [B,N,3], "xyz2" [B,S,3], "points1" [B,D1,N] (absent when D1 = 0), "points2" [B,D2,S];
  - the seeded state_dict "sd:<key>" with "keys": running statistics away from their identity start and BatchNorm weights of BOTH
    signs (a negative weight flips a channel: the fold must carry the sign into Wf);
  - the eval-mode output "ev_out" [B,mlp[-1],N].
Coordinates are integer multiples of 2^-10 in [-1, 1), where the reference's expanded distance form is exact and equals the contract's
difference form.  While writing it asserts, and moves on to the next seed where one fails,
  - no distance tie among a point's first four candidates, and the restated three_nn (tests/propagate_ref) gives the three indices the
    reference's sort gives,
  - every layer has BatchNorm weights of both signs,
  - the reference's fp32 run and its float64 run agree within 1e-4 under tests.common.compare_case, a tenth of the tolerance the tests
    use: no ReLU kink sits on a knife edge,
  - tests/fp_fused_ref.py's chain on the folded state_dict agrees with the recorded output within 1e-3.
The seed a case ends on is printed; tests/fp_fused_ref.GOLDEN_CASES must name it (the maker refuses to write otherwise).
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fp_fused_ref as R           # noqa: E402
from tests import propagate_ref as P          # noqa: E402
from tests.common import compare_case         # noqa: E402


def ref_module(name, rel):
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cf(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _run(U, state, case, q, r, f1, f2, dtype):
    _, B, N, S, D1, D2, mlp = case
    mod = U.PointNetFeaturePropagation(D1 + D2, list(mlp))
    mod.load_state_dict(state, strict=True)
    mod.to(dtype).eval()
    with torch.no_grad():
        out = mod(_cf(q.transpose(0, 2, 1), dtype), _cf(r.transpose(0, 2, 1), dtype), None if f1 is None else _cf(f1, dtype), _cf(f2, dtype))
    return {"out:new_points": out.numpy().astype(np.float64)}


def attempt(U, name, seed):
    case = R.GOLDEN_CASES[name]
    _, B, N, S, D1, D2, mlp = case
    q, r, f1, f2 = R.golden_inputs(name, seed)
    for x in (q, r):
        assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    if not P.distinct_smallest(q, r, 4):
        return "a distance tie among a point's first four candidates"
    idx, _, w = P.three_nn_batch(q, r)
    if S > 1:
        with torch.no_grad():
            order = U.square_distance(torch.from_numpy(q), torch.from_numpy(r)).sort(dim=-1)[1][:, :, :3].numpy()
        if not np.array_equal(order, idx[:, :, :order.shape[2]]):
            return "the restated three_nn and the reference's sort disagree"
    torch.manual_seed(seed)
    mod = U.PointNetFeaturePropagation(D1 + D2, list(mlp))
    for bn in mod.mlp_bns:
        torch.nn.init.uniform_(bn.weight, -1.5, 1.5)
        torch.nn.init.uniform_(bn.bias, -0.5, 0.5)
        torch.nn.init.uniform_(bn.running_mean, -0.25, 0.25)
        torch.nn.init.uniform_(bn.running_var, 0.5, 1.5)
        if not (bool((bn.weight > 0).any()) and bool((bn.weight < 0).any())):
            return "a BatchNorm whose weights have one sign"
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    r32, r64 = (_run(U, {k: v.clone() for k, v in state.items()}, case, q, r, f1, f2, dt) for dt in (torch.float32, torch.float64))
    try:
        worst = compare_case(r32, r64, 1e-4, name + ": fp32 against float64")
    except AssertionError as e:
        return str(e)
    print("  %s seed %d: module, eval: fp32 against float64 worst %.3e at %s" % ((name, seed) + tuple(worst)))
    layers = R.fold_state({k: v.numpy() for k, v in state.items()}, R.single_prefixes(len(mlp)), eps=float(mod.mlp_bns[0].eps))
    chain = R.level_batch(idx, w, f2, f1, layers)
    try:
        worst = compare_case({"out:new_points": chain}, r32, 1e-3, name + ": the restatement")
    except AssertionError as e:
        return str(e)
    print("  %s: the restatement against the recorded output: worst %.3e" % (name, worst[0]))
    assert float(r32["out:new_points"].max()) > 0
    out = {name + "_xyz1": q, name + "_xyz2": r, name + "_points2": f2, name + "_ev_out": r32["out:new_points"].astype(np.float32)}
    if f1 is not None:
        out[name + "_points1"] = f1
    for k, v in state.items():
        out["%s_sd:%s" % (name, k)] = v.numpy()
    out[name + "_keys"] = np.array(list(state))
    return out


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    out = {}
    for name, case in R.GOLDEN_CASES.items():
        for seed in range(case[0], case[0] + 20):
            res = attempt(U, name, seed)
            if isinstance(res, dict):
                break
            print("  %s seed %d refused: %s" % (name, seed, res))
        else:
            sys.exit("%s: no seed passed" % name)
        if seed != case[0]:
            sys.exit("%s: seed %d passes, tests/fp_fused_ref.GOLDEN_CASES names %d - put %d there and run again" % (name, seed, case[0], seed))
        out.update(res)
    path = os.path.join(HERE, "fp_fused.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "msg.npz"))


if __name__ == "__main__":
    main()
