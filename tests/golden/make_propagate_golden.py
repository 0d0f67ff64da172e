#!/usr/bin/env python3
"""Generate tests/golden/propagate.npz: the REFERENCE's feature propagation on small lattice inputs, recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_propagate_golden          (from the repo root, CPU)

It runs `PointNetFeaturePropagation(D, [])(xyz1, xyz2, None, points2)` of models/utils/pointnet_util.py:270-320 (no MLP: the
interpolation alone) on the cases of tests/propagate_ref.GOLDEN_CASES and stores, per case, the inputs "<name>_q" [B,P,3], "<name>_r"
[B,N,3], "<name>_f" [B,D,N], the reference's output "<name>_out" [B,D,P] and, for N >= 3, its neighbours "<name>_idx" [B,P,3] =
`square_distance(xyz1, xyz2).sort(-1)[1][..., :3]`.  Coordinates are integer multiples of 2^-10 in [-1, 1), where the reference's
expanded distance form is exact and equals the contract's difference form; half of the sampled points are copies of queries.  Only
data is stored, no reference source.  While writing it asserts
  - every query's four smallest distances are distinct, so the reference's unspecified sort order never enters,
  - `square_distance` equals tests/propagate_ref.distances bit for bit,
  - the restatement tests/propagate_ref gives the recorded neighbours and output bit for bit (tests/test_host_propagate.py asserts
    that again from the file).
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import propagate_ref as R        # noqa: E402


def ref_module(name, rel):
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    out = {}
    for name, (seed, B, P, N, D) in R.GOLDEN_CASES.items():
        q, r, f = R.lattice_case(seed, B, P, N, D)
        assert R.distinct_smallest(q, r), "%s: a query has a tie among its four smallest distances - pick another seed" % name
        tq, tr, tf = torch.from_numpy(q), torch.from_numpy(r), torch.from_numpy(f)
        with torch.no_grad():
            got = U.PointNetFeaturePropagation(D, [])(tq.permute(0, 2, 1), tr.permute(0, 2, 1), None, tf).contiguous().numpy()
            sq = U.square_distance(tq, tr)
        assert got.shape == (B, D, P) and got.dtype == np.float32
        for b in range(B):
            assert np.array_equal(sq[b].numpy().view(np.uint32), R.distances(q[b], r[b]).view(np.uint32)), "%s: distance forms differ" % name
        mine = R.propagate_batch(q, r, f)
        assert np.array_equal(mine.view(np.uint32), got.view(np.uint32)), "%s: the restatement differs from the reference" % name
        out[name + "_q"], out[name + "_r"], out[name + "_f"], out[name + "_out"] = q, r, f, got
        if N >= 3:
            idx = sq.sort(-1)[1][..., :3].numpy().astype(np.int64)
            assert np.array_equal(idx, R.three_nn_batch(q, r)[0]), "%s: the restatement's neighbours differ from the reference's" % name
            out[name + "_idx"] = idx
        coincident = int(sum((R.distances(q[b], r[b]).min(axis=1) == 0).sum() for b in range(B)))
        print("  %-6s B %d P %4d N %4d D %d   %d queries coincide with a sampled point" % (name, B, P, N, D, coincident))
    path = os.path.join(HERE, "propagate.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
