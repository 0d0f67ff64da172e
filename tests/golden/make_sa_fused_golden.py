#!/usr/bin/env python3
"""Generate tests/golden/sa_fused.npz: the REFERENCE's single-scale set-abstraction level in eval mode on small lattice inputs,
recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_sa_fused_golden          (from the repo root, CPU)

For tests/sa_fused_ref.GOLDEN_CASE - B 2, N 256, S 32, radius 0.25, nsample 16, D 4, widths (8, 12, 16) - it runs
`PointNetSetAbstraction(S, radius, nsample, D + 3, mlp, False)` of the reference's models/utils/pointnet_util.py in eval mode and
stores data only, no reference source:
  - the inputs "xyz" [B,N,3], "points" [B,N,D] and the start "start" [B] that torch.randint draws first under torch.manual_seed(seed);
  - the centres "new_xyz" [B,S,3] and the reference's `query_ball_point` "idx" [B,S,nsample];
  - the seeded state_dict "sd:<key>" with "keys" / "shapes": running statistics away from their identity start and BatchNorm weights
    of BOTH signs (a negative weight flips a channel: the fold must carry the sign into Wf);
  - the eval-mode outputs "ev_out:new_xyz" [B,3,S] and "ev_out:new_points" [B,mlp[-1],S].
Coordinates are integer multiples of 2^-10 in [-1, 1), where the reference's expanded distance form is exact and equals the contract's
difference form.  While writing it asserts
  - the restatements (tests/fps_ref, tests/group_ref) reproduce the reference's centres and indices exactly, no group is empty, and
    there are full groups and padded ones,
  - every layer has BatchNorm weights of both signs,
  - the reference's fp32 run and its float64 run agree within 1e-4 under tests.common.compare_case, a tenth of the tolerance the tests
    use: no ReLU kink or max tie sits on a knife edge; if they do not, pick another seed,
  - tests/sa_fused_ref.py's chain on the folded state_dict agrees with the recorded output within 1e-3.
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fps_ref as F                # noqa: E402
from tests import group_ref as G              # noqa: E402
from tests import sa_fused_ref as R           # noqa: E402
from tests.common import compare_case         # noqa: E402


def ref_module(name, rel):
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(U, state, x, pts, dtype):
    seed, B, N, S, radius, nsample, D, mlp = R.GOLDEN_CASE
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                      # the reference's sampling builds its distance table in the default dtype
    try:
        mod = U.PointNetSetAbstraction(S, radius, nsample, D + 3, list(mlp), False)
        mod.load_state_dict(state, strict=True)
        mod.to(dtype).eval()
        tx = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dtype)
        tp = torch.from_numpy(np.ascontiguousarray(pts.transpose(0, 2, 1))).to(dtype)
        torch.manual_seed(seed)
        with torch.no_grad():
            new_xyz, new_points = mod(tx, tp)
        return {"out:new_xyz": new_xyz.numpy().astype(np.float64), "out:new_points": new_points.numpy().astype(np.float64)}
    finally:
        torch.set_default_dtype(old)


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    seed, B, N, S, radius, nsample, D, mlp = R.GOLDEN_CASE
    torch.manual_seed(seed)
    start = torch.randint(0, N, (B,), dtype=torch.long).numpy().astype(np.int64)
    x, pts = R.golden_inputs()
    assert x.shape == (B, N, 3) and np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    tx = torch.from_numpy(x)
    torch.manual_seed(seed)
    with torch.no_grad():
        fps_idx = U.farthest_point_sample(tx, S)
        new_xyz = U.index_points(tx, fps_idx)
        idx = U.query_ball_point(radius, nsample, tx, new_xyz)
    fps_idx, new_xyz, idx = fps_idx.numpy().astype(np.int64), np.ascontiguousarray(new_xyz.numpy()), idx.numpy().astype(np.int64)
    assert np.array_equal(fps_idx[:, 0], start) and np.array_equal(F.fps_batch(x, S, start), fps_idx)
    mine, count = G.query_ball_batch(x, new_xyz, G.r2_of(radius), nsample)
    assert np.array_equal(mine, idx) and (count >= 1).all()
    full, padded = int((count == nsample).sum()), int((count < nsample).sum())
    assert full >= 1 and padded >= 1, (full, padded)
    print("  counts %d..%d, %d of %d groups full" % (count.min(), count.max(), full, count.size))

    torch.manual_seed(seed)
    mod = U.PointNetSetAbstraction(S, radius, nsample, D + 3, list(mlp), False)
    for bn in mod.mlp_bns:
        torch.nn.init.uniform_(bn.weight, -1.5, 1.5)
        torch.nn.init.uniform_(bn.bias, -0.5, 0.5)
        torch.nn.init.uniform_(bn.running_mean, -0.25, 0.25)
        torch.nn.init.uniform_(bn.running_var, 0.5, 1.5)
        assert bool((bn.weight > 0).any()) and bool((bn.weight < 0).any())
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    r32, r64 = (_run(U, {k: v.clone() for k, v in state.items()}, x, pts, dt) for dt in (torch.float32, torch.float64))
    worst = compare_case(r32, r64, 1e-4, "fp32 against float64")
    print("  module, eval: fp32 against float64 worst %.3e at %s" % worst)
    assert np.array_equal(np.ascontiguousarray(r32["out:new_xyz"].transpose(0, 2, 1)).astype(np.float32).view(np.uint32), new_xyz.view(np.uint32))
    layers = R.fold_state({k: v.numpy() for k, v in state.items()}, R.single_prefixes(len(mlp)), eps=float(mod.mlp_bns[0].eps))
    chain = R.level_batch(x, new_xyz, idx, pts, layers)
    worst = compare_case({"out:new_points": chain}, {"out:new_points": r32["out:new_points"]}, 1e-3, "the restatement")
    print("  the restatement against the recorded output: worst %.3e" % worst[0])
    assert float(r32["out:new_points"].max()) > 0

    out = {"xyz": x, "points": pts, "start": start, "new_xyz": new_xyz, "idx": idx.astype(np.int16)}
    for k, v in state.items():
        out["sd:" + k] = v.numpy()
    for k, v in r32.items():
        out["ev_" + k] = v.astype(np.float32)
    out["keys"] = np.array(list(state))
    out["shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in state.values()], dtype=np.int64)
    path = os.path.join(HERE, "sa_fused.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "msg.npz"))


if __name__ == "__main__":
    main()
