"""Times of farthest point sampling on the GPU (svnet_amd/data.py farthest_point_sample, csrc/fps.hip), HIP events around the call:

  1. the sampler launch at (M, P, npoint) = (64, 10000, 1024) - ModelNet40_v2(uniform=True)'s shape - and (256, 2048, 1024);
  2. at the same shapes, the reference's loop (models/utils/pointnet_util.py:63-84) restated with torch operations on the device:
     what a user has without the kernel.  Written here from the semantics in svnet_amd/data.py's docstring: per iteration a gather
     of the centroids, a broadcast subtraction, a squared sum, a minimum and an argmax - npoint dependent rounds of small launches.
     It is a timing yardstick, not a bit-exact twin (torch's reductions may order and tie differently); the tool prints how many
     indices agree.

Both legs run in this one process, alternating, after a warm-up of each shape.

    python tools/time_fps.py [--out profiles/fps_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

SHAPES = ((64, 10000, 1024), (256, 2048, 1024))


def torch_ops_fps(torch, xyz, npoint, start):
    B, P, _ = xyz.shape
    idx = torch.empty(B, npoint, dtype=torch.int64, device=xyz.device)
    mind = torch.full((B, P), 1e10, dtype=torch.float32, device=xyz.device)
    rows = torch.arange(B, device=xyz.device)
    f = start.clone()
    for i in range(npoint):
        idx[:, i] = f
        d = xyz - xyz[rows, f].view(B, 1, 3)
        mind = torch.minimum(mind, (d * d).sum(-1))
        f = mind.argmax(-1)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_fps.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import _lib, _pointset, synth
    from svnet_amd.data import farthest_point_sample, fps_start
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    for M, P, npoint in SHAPES:
        xyz = torch.from_numpy(np.ascontiguousarray(synth.normal(90 + P, 0, (M, P, 3)))).to(dev)
        start = torch.from_numpy(fps_start(1, M, P)).to(dev)
        idx = torch.empty(M, npoint, dtype=torch.int64, device=dev)

        def kernel():            # the entry point alone: no start check, no allocation
            _pointset.fps_launch(xyz, M, P, npoint, start, idx)
            return idx

        def whole():             # what a caller pays: + the start range check (one reduction, one synchronisation) and the allocation
            return farthest_point_sample(xyz, npoint, start)

        def ops():
            return torch_ops_fps(torch, xyz, npoint, start)
        for fn in (kernel, whole, ops):
            fn()
        torch.cuda.synchronize()
        res = {"kernel": [], "whole": [], "ops": []}
        for _ in range(args.reps):               # alternating legs
            for name, fn in (("kernel", kernel), ("whole", whole), ("ops", ops)):
                t, out = timed(torch, fn, 1)
                res[name].append(t)
                if name == "kernel":
                    mine = out.clone()
                elif name == "ops":
                    agree = float((out == mine).float().mean())
        med = {k: median(v) for k, v in res.items()}
        tag = "M %3d P %5d npoint %4d  (tier %d)" % (M, P, npoint, _lib.lib().svnet_fps_tier(P))
        for name, label in (("kernel", "svnet_fps_f32 alone        "), ("whole", "farthest_point_sample()    "),
                            ("ops", "torch ops on the device    ")):
            lines.append("%s  %s %10.3f ms (median of %d; %s)" % (tag, label, med[name], args.reps, " ".join("%.3f" % v for v in res[name])))
        lines.append("%s  torch ops / kernel = %.1f x;  %.2f us per iteration per cloud-wave of the kernel;  %.4f of the indices agree"
                     % (tag, med["ops"] / med["kernel"], med["kernel"] * 1e3 / npoint / (-(-M // 256)), agree))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
