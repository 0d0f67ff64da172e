#!/usr/bin/env python3
"""Generate tests/golden/fps.npz: the REFERENCE's farthest point sampling and pc_normalize on small procedural inputs, recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_fps_golden          (from the repo root, CPU)

It calls `farthest_point_sample` of models/utils/pointnet_util.py:63-84 under torch.manual_seed on the clouds of
tests/fps_ref.golden_cases() and stores the index lists "fps_<name>" [M,npoint] (column 0 is the start torch.randint drew), and
`pc_normalize` of data.py:15-20 on the selections of tests/fps_ref.norm_cases() ("norm_<name>" [N,3] float32).  Inputs are procedural
and not stored; no reference source is stored.  While writing it asserts what tests/test_host_fps.py asserts again: the restatement
tests/fps_ref.fps gives every list bit for bit, and the float64 normalisation is within fps_ref.bound_numpy_f32 of the recorded one.
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fps_ref as F        # noqa: E402


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
    try:
        import h5py        # noqa: F401
    except ImportError:    # data.py imports it at module level; pc_normalize does not use it
        sys.modules["h5py"] = types.ModuleType("h5py")
    D = ref_module("ref_data", "data.py")
    out = {}
    for k, (name, (clouds, npoint)) in enumerate(F.golden_cases().items()):
        torch.manual_seed(100 + k)
        idx = U.farthest_point_sample(torch.from_numpy(clouds), npoint).numpy().astype(np.int64)
        assert idx.shape == (clouds.shape[0], npoint)
        mine = F.fps_batch(clouds, npoint, idx[:, 0])
        assert np.array_equal(mine, idx), "%s: the restatement differs from the reference" % name
        out["fps_" + name] = idx
        print("  fps_%-12s M %d P %5d npoint %4d  starts %s" % (name, clouds.shape[0], clouds.shape[1], npoint, idx[:, 0].tolist()))
    for name, sel in F.norm_cases().items():
        got = D.pc_normalize(sel)
        assert got.dtype == np.float32 and got.shape == sel.shape and sel.shape[0] <= 128
        err, bound = float(abs(F.normalize_f64(sel) - got).max()), F.bound_numpy_f32(sel)
        own = float(abs(F.normalize_f64(sel) - F.normalize_f32(sel)).max())
        assert err <= bound, (name, err, bound)
        assert own <= F.bound_f32(sel), (name, own, F.bound_f32(sel))
        out["norm_" + name] = got
        print("  norm_%-14s N %3d  |f64 - reference| %.3e (bound %.3e)   |f64 - fp32 restatement| %.3e (bound %.3e)"
              % (name, sel.shape[0], err, bound, own, F.bound_f32(sel)))
    path = os.path.join(HERE, "fps.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
