#!/usr/bin/env python3
"""Generate tests/golden/sa_global.npz: the REFERENCE's global set-abstraction level (group_all) in eval mode on small lattice inputs,
recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_sa_global_golden          (from the repo root, CPU)

For tests/sa_global_ref.GOLDEN_CASE - B 2, N 40, D 5, widths (12, 16, 260): one width past 256, N no multiple of 16 - it runs
`PointNetSetAbstraction(None, None, None, D + 3, mlp, True)` of the reference's models/utils/pointnet_util.py in eval mode and stores
data only, no reference source:
  - the inputs "xyz" [B,3,N] and "points" [B,D,N], channel-first as the module receives them;
  - the seeded state_dict "sd:<key>" with "keys" / "shapes": running statistics away from their identity start and BatchNorm weights
    of BOTH signs (a negative weight flips a channel: the fold must carry the sign into Wf);
  - the eval-mode outputs "ev_out:new_xyz" [B,3,1] and "ev_out:new_points" [B,mlp[-1],1].
Coordinates are integer multiples of 2^-10 in [-1, 1).  While writing it asserts
  - every layer has BatchNorm weights of both signs, and new_xyz is exact zeros,
  - the reference's fp32 run and its float64 run agree within 1e-4 under tests.common.compare_case, a tenth of the tolerance the tests
    use: no ReLU kink or max tie sits on a knife edge; if they do not, pick another seed,
  - tests/sa_global_ref.py's chain on the folded state_dict agrees with the recorded output within 1e-3,
  - the file is smaller than msg.npz.
No test imports the reference: they read the .npz only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import sa_fused_ref as R                          # noqa: E402
from tests import sa_global_ref as SG                        # noqa: E402
from tests.common import compare_case                        # noqa: E402
from tests.golden.make_sa_fused_golden import ref_module     # noqa: E402


def _run(U, state, x, pts, dtype):
    seed, B, N, D, mlp = SG.GOLDEN_CASE
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                      # the reference's zeros for new_xyz are of the default dtype
    try:
        mod = U.PointNetSetAbstraction(None, None, None, D + 3, list(mlp), True)
        mod.load_state_dict(state, strict=True)
        mod.to(dtype).eval()
        with torch.no_grad():
            new_xyz, new_points = mod(torch.from_numpy(x).to(dtype), torch.from_numpy(pts).to(dtype))
        return {"out:new_xyz": new_xyz.numpy().astype(np.float64), "out:new_points": new_points.numpy().astype(np.float64)}
    finally:
        torch.set_default_dtype(old)


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    seed, B, N, D, mlp = SG.GOLDEN_CASE
    x, pts = SG.golden_inputs()
    assert x.shape == (B, 3, N) and pts.shape == (B, D, N) and np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
    assert N % 16 and max(mlp) > 256

    torch.manual_seed(seed)
    mod = U.PointNetSetAbstraction(None, None, None, D + 3, list(mlp), True)
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
    assert r32["out:new_xyz"].shape == (B, 3, 1) and not r32["out:new_xyz"].any() and r32["out:new_points"].shape == (B, mlp[-1], 1)
    layers = R.fold_state({k: v.numpy() for k, v in state.items()}, R.single_prefixes(len(mlp)), eps=float(mod.mlp_bns[0].eps))
    chain = SG.level_batch(x, pts, layers)
    worst = compare_case({"out:new_points": chain}, {"out:new_points": r32["out:new_points"]}, 1e-3, "the restatement")
    print("  the restatement against the recorded output: worst %.3e" % worst[0])
    assert float(r32["out:new_points"].max()) > 0

    out = {"xyz": x, "points": pts}
    for k, v in state.items():
        out["sd:" + k] = v.numpy()
    for k, v in r32.items():
        out["ev_" + k] = v.astype(np.float32)
    out["keys"] = np.array(list(state))
    out["shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in state.values()], dtype=np.int64)
    path = os.path.join(HERE, "sa_global.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "msg.npz"))


if __name__ == "__main__":
    main()
