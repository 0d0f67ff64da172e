#!/usr/bin/env python3
"""Generate tests/golden/group.npz: the REFERENCE's ball query and grouping on small lattice inputs, recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_group_golden          (from the repo root, CPU)

For every case of tests/group_ref.GOLDEN_CASES it runs `sample_and_group(npoint, radius, nsample, xyz, points, returnfps=True)` of
models/utils/pointnet_util.py:110-143 under torch.manual_seed(seed) (the start of its sampling is what torch.randint draws first
under that seed; it is recorded), and `query_ball_point(radius, nsample, xyz, new_xyz)` (lines 87-107) on the centres that gave.
Stored per case: the inputs "<name>_xyz", "<name>_points" (D > 0), "<name>_start" and the results "<name>_fps", "<name>_new_xyz",
"<name>_idx", "<name>_new_points", "<name>_grouped_xyz" (tests/group_ref.py lists the shapes).  Coordinates are integer multiples of
2^-10 in [-1, 1), where the reference's expanded distance form is exact and equals the contract's difference form; every centre is
a point of its cloud.  Only data is stored, no reference source.  While writing it asserts
  - `square_distance` equals tests/group_ref.distances bit for bit,
  - the restatement (tests/fps_ref.fps_batch for the sampling, tests/group_ref for the rest) reproduces the reference's sampled
    indices, ball-query indices, new_points and grouped_xyz bit for bit,
  - no recorded group is empty, and both full groups (cut at nsample) and partial ones (padded) occur,
  - for the radii whose square is exact in fp32 (0.125, 0.25, 0.5) at least one recorded group contains a point at distance exactly
    r2: on the sphere is inside.
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fps_ref as F        # noqa: E402
from tests import group_ref as G      # noqa: E402


def ref_module(name, rel):
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    out, full, partial = {}, 0, 0
    for name, (seed, B, N, S, nsample, D, radius) in G.GOLDEN_CASES.items():
        torch.manual_seed(seed)
        start = torch.randint(0, N, (B,), dtype=torch.long).numpy().astype(np.int64)     # the sampling's first draw under this seed
        x, pts = G.golden_inputs(name, start)
        assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
        tx, tp = torch.from_numpy(x), None if pts is None else torch.from_numpy(pts)
        torch.manual_seed(seed)
        with torch.no_grad():
            new_xyz, new_points, grouped_xyz, fps_idx = U.sample_and_group(S, radius, nsample, tx, tp, returnfps=True)
            idx = U.query_ball_point(radius, nsample, tx, new_xyz)
            sq = U.square_distance(new_xyz, tx)
        fps_idx, idx = fps_idx.numpy().astype(np.int64), idx.numpy().astype(np.int64)
        new_xyz, new_points, grouped_xyz = (np.ascontiguousarray(t.numpy()) for t in (new_xyz, new_points, grouped_xyz))
        assert np.array_equal(fps_idx[:, 0], start), "%s: the sampling did not start where torch.randint was expected to point" % name
        assert new_points.shape == (B, S, nsample, 3 + D) and new_points.dtype == np.float32 and idx.shape == (B, S, nsample)

        r2 = G.r2_of(radius)
        assert np.array_equal(F.fps_batch(x, S, start), fps_idx), "%s: the sampling restatement differs from the reference" % name
        assert np.array_equal(_bits(new_xyz), _bits(np.stack([x[b, fps_idx[b]] for b in range(B)])))
        on_sphere = 0
        for b in range(B):
            dist = G.distances(new_xyz[b], x[b])
            assert np.array_equal(sq[b].numpy().view(np.uint32), dist.view(np.uint32)), "%s: distance forms differ" % name
            on_sphere += int((np.take_along_axis(dist, idx[b], axis=1) == r2).any(axis=1).sum())
        mine_idx, count = G.query_ball_batch(x, new_xyz, r2, nsample)
        assert np.array_equal(mine_idx, idx), "%s: the restatement's indices differ from the reference's" % name
        assert (count >= 1).all(), "%s: an empty group" % name
        assert np.array_equal(_bits(G.group_batch(x, new_xyz, idx, pts)), _bits(new_points)), "%s: new_points differ" % name
        assert np.array_equal(_bits(np.stack([x[b][idx[b]] for b in range(B)])), _bits(grouped_xyz)), "%s: grouped_xyz differ" % name
        if radius in G.EXACT_RADII:
            assert float(r2) == radius * radius and on_sphere >= 1, "%s: no recorded group holds a point at distance exactly r2" % name
        else:
            assert float(r2) * 2 ** 20 != round(float(r2) * 2 ** 20) and on_sphere == 0      # no lattice distance equals this r2
        full += int((count == nsample).sum())
        partial += int((count < nsample).sum())

        out[name + "_xyz"], out[name + "_start"], out[name + "_fps"], out[name + "_new_xyz"] = x, start, fps_idx, new_xyz
        out[name + "_idx"], out[name + "_new_points"], out[name + "_grouped_xyz"] = idx, new_points, grouped_xyz
        if pts is not None:
            out[name + "_points"] = pts
        print("  %-6s B %d N %4d S %3d nsample %2d D %d radius %-5g  counts %2d..%2d, %3d of %3d groups full, %d hold a point on the sphere"
              % (name, B, N, S, nsample, D, radius, count.min(), count.max(), int((count == nsample).sum()), count.size, on_sphere))
    assert full >= 1 and partial >= 1, "the cases must hold full groups (the cut) and partial ones (the padding): %d / %d" % (full, partial)
    path = os.path.join(HERE, "group.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
