"""Times of the ball query and the grouping on the GPU (svnet_amd/group.py, csrc/group.hip), HIP events around repeated launches:

  1. svnet_ball_query_f32 alone, svnet_group_points_f32 alone, and sample_and_group without its farthest point sampling (gather of
     the centres + Grouper.run: fixed buffers) at
         (B, N, S, radius, nsample, D) = (32, 1024, 512, 0.2, 32, 0) and (32, 2048, 512, 0.4, 64, 64)
     - the first set-abstraction level of a PointNet++ classifier and a wider one with attributes - on DevicePool.synthetic clouds,
     the centres sampled from them by farthest point sampling;
  2. at the same shapes, the reference's formulation (models/utils/pointnet_util.py:87-143) restated with torch operations on the
     device: what a user has without the kernels, and the thing being replaced, so the ratio is the number to report.  Written here
     from the contract in svnet_amd/group.py's docstring: the [B,S,N] distance matrix (difference form), arange(N) masked to N where
     outside, a full sort along N, the first nsample columns, the padding mask, and advanced indexing for the gathers.  It runs at
     the largest batch that fits (halved on an out-of-memory error, the time scaled to B clouds); the tool counts the indices and
     output words in which it differs from the kernels (0 expected: same distance form, single-rounded operations).

Legs alternate inside this one process after a warm-up of each shape.  The output write of the grouping (B S nsample (3 + D) 4 bytes)
over its time is reported as a fraction of the 8 TB/s HBM peak, and from the indices and counts the mean fraction of the N points a
wave of the ball query looks at before it leaves its loop (a full group ends with the 64-candidate step that holds its last index).

    python tools/time_group.py [--out profiles/group_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

SHAPES = ((32, 1024, 512, 0.2, 32, 0), (32, 2048, 512, 0.4, 64, 64))
HBM_PEAK = 8.0e12


def torch_ops_query(torch, xyz, new_xyz, r2, nsample):
    """[B,N,3], [B,S,3] -> idx [B,S,nsample] int64 with torch operations only."""
    B, N, S = xyz.shape[0], xyz.shape[1], new_xyz.shape[1]
    d = new_xyz[:, :, None, 0] - xyz[:, None, :, 0]
    dist = d * d
    d = new_xyz[:, :, None, 1] - xyz[:, None, :, 1]
    dist += d * d
    d = new_xyz[:, :, None, 2] - xyz[:, None, :, 2]
    dist += d * d
    del d
    idx = torch.arange(N, dtype=torch.int64, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    idx[dist > r2] = N
    del dist
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, 0:1].repeat(1, 1, nsample)
    pad = idx == N
    idx[pad] = first[pad]
    return idx


def torch_ops_group(torch, xyz, new_xyz, idx, points):
    """-> [B,S,nsample,3+D] with advanced indexing, a subtraction and a cat."""
    B = xyz.shape[0]
    batch = torch.arange(B, dtype=torch.int64, device=xyz.device).view(B, 1, 1)
    centred = xyz[batch, idx, :] - new_xyz[:, :, None, :]
    return centred if points is None else torch.cat([centred, points[batch, idx, :]], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_group.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import synth
    from svnet_amd import group as Gr
    from svnet_amd.data import DevicePool, farthest_point_sample, fps_start
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for B, N, S, radius, nsample, D in SHAPES:
        xyz = DevicePool.synthetic(400 + N, B, N, 16, device=dev).data
        points = torch.from_numpy(np.ascontiguousarray(synth.normal(400 + N, 1, (B, N, D)))).to(dev) if D else None
        fps_idx = farthest_point_sample(xyz, S, torch.from_numpy(fps_start(1, B, N)).to(dev))
        gather_index = fps_idx.unsqueeze(2).expand(-1, -1, 3)
        new_xyz = torch.gather(xyz, 1, gather_index).contiguous()
        grouper = Gr.Grouper(B, N, S, nsample, D, dev)
        r2 = Gr._r2(radius)

        def query():
            Gr._query_launch(xyz, new_xyz, B, N, S, r2, nsample, grouper.idx, grouper.count)

        def group():
            Gr._group_launch(xyz, new_xyz, points, grouper.idx, B, N, S, nsample, D, grouper.out)

        def both():
            return grouper.run(xyz, torch.gather(xyz, 1, gather_index), radius, points)

        tb = B
        while True:                                        # the largest batch the torch restatement fits
            try:
                torch_ops_group(torch, xyz[:tb], new_xyz[:tb], torch_ops_query(torch, xyz[:tb], new_xyz[:tb], r2, nsample),
                                None if points is None else points[:tb])
                torch.cuda.synchronize()
                break
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
                if tb == 1:
                    raise
                tb //= 2
        pts_tb = None if points is None else points[:tb]
        ops_idx = torch_ops_query(torch, xyz[:tb], new_xyz[:tb], r2, nsample)

        def ops_query():
            return torch_ops_query(torch, xyz[:tb], new_xyz[:tb], r2, nsample)

        def ops_group():
            return torch_ops_group(torch, xyz[:tb], new_xyz[:tb], ops_idx, pts_tb)

        def ops_both():
            c = torch.gather(xyz[:tb], 1, gather_index[:tb])
            return torch_ops_group(torch, xyz[:tb], c, torch_ops_query(torch, xyz[:tb], c, r2, nsample), pts_tb)

        legs = (("query", query, args.inner), ("group", group, args.inner), ("both", both, args.inner),
                ("ops_query", ops_query, 2), ("ops_group", ops_group, 2), ("ops_both", ops_both, 2))
        for _, fn, _ in legs:
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _, _ in legs}
        for _ in range(args.reps):
            for name, fn, inner in legs:
                t, out = timed(torch, fn, inner)
                res[name].append(t * (B / tb if name.startswith("ops") else 1.0))
                if name == "both":
                    mine = out.clone()
                elif name == "ops_query":
                    idx_diff = int((out != grouper.idx[:tb]).sum())
                elif name == "ops_both":
                    out_diff = int((out.contiguous().view(torch.int32) != mine[:tb].contiguous().view(torch.int32)).sum())
        med = {k: median(v) for k, v in res.items()}
        tag = "B %d N %d S %d r %g nsample %d D %d" % (B, N, S, radius, nsample, D)
        labels = (("query", "svnet_ball_query_f32               "), ("group", "svnet_group_points_f32             "),
                  ("both", "gather + Grouper.run (fixed buf)   "), ("ops_query", "torch ops query, batch %2d, scaled  " % tb),
                  ("ops_group", "torch ops group, batch %2d, scaled  " % tb), ("ops_both", "torch ops gather + both, scaled     "))
        for name, label in labels:
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[name], " ".join("%.3f" % v for v in res[name])))
        lines.append("%s  torch ops / kernels: query %.1f x;  group %.1f x;  gather + both %.1f x;  differing indices %d, differing output words %d"
                     % (tag, med["ops_query"] / med["query"], med["ops_group"] / med["group"], med["ops_both"] / med["both"], idx_diff, out_diff))
        count, last = grouper.count.to(torch.int64), grouper.idx[:, :, nsample - 1]
        seen = torch.where(count >= nsample, torch.clamp((last // 64 + 1) * 64, max=N), torch.full_like(last, N))
        out_bytes = B * S * nsample * (3 + D) * 4
        lines.append("%s  groups: %.1f %% full, %.1f %% empty, mean count %.1f;  a wave scans %.3f of N on average;  out write %.1f MB: "
                     "%.2f TB/s = %.2f of the 8 TB/s HBM peak (grouping alone)"
                     % (tag, 100.0 * float((count >= nsample).float().mean()), 100.0 * float((count == 0).float().mean()),
                        float(count.float().mean()), float(seen.float().mean()) / N, out_bytes / 1e6,
                        out_bytes / (med["group"] * 1e-3) / 1e12, out_bytes / (med["group"] * 1e-3) / HBM_PEAK))
        del xyz, points, new_xyz, grouper, ops_idx
        torch.cuda.empty_cache()
    emit(lines, args.out)


if __name__ == "__main__":
    main()
