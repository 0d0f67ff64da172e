"""Times of the multi-scale grouping on the GPU (svnet_amd/group.py, csrc/group.hip) against the single-scale
calls it replaces, HIP events around repeated launches, at

    (B, N, S, radii, nsample, D) = (32, 1024, 512, 0.1/0.2/0.4, 16/32/128, 0), (32, 512, 128, 0.2/0.4/0.8, 32/64/128, 320) and
                                   (32, 2048, 512, 0.1/0.2/0.4, 32/64/128, 6)

- the first two levels of a PointNet++ MSG classifier and a wider first level with attributes - on DevicePool.synthetic clouds, the
centres sampled from them by farthest point sampling.  Three pairs of legs, every buffer allocated before the clock starts:

  1. svnet_ball_query_msg_f32, one pass, against R calls of svnet_ball_query_f32;
  2. svnet_group_points_msg_f32, one launch, against R calls of svnet_group_points_f32;
  3. group_points_msg_backward (the reverse lists of the concatenated table + one sum) against R calls of group_points_backward (R list
     builds, R sums) plus the R - 1 adds of their results; only where D > 0.

The yardstick is the R-call path in the same process on the same machine: legs alternate after a warm-up of each shape, the median of
the rounds is reported with every round listed.  The tool counts the indices in which the two queries differ and the words in which
the two groupings differ after rotating the columns (0 expected), and gives the largest difference of the two backwards (their sum
orders differ: scale-major per centre here, scale after scale there).  From the indices and counts: the mean fraction of the N points
a wave looks at before it leaves a centre, per scale - what the single-scale query scans - and for their union, what the one-pass
query scans (a full list ends with the 64-candidate step that holds its last index).

    python tools/time_msg.py [--out profiles/msg_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

SHAPES = ((32, 1024, 512, (0.1, 0.2, 0.4), (16, 32, 128), 0),
          (32, 512, 128, (0.2, 0.4, 0.8), (32, 64, 128), 320),
          (32, 2048, 512, (0.1, 0.2, 0.4), (32, 64, 128), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_msg.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import synth
    from svnet_amd import group as Gr
    from svnet_amd.data import DevicePool, farthest_point_sample, fps_start
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for B, N, S, radii, nsamples, D in SHAPES:
        R, Ktot = len(radii), sum(nsamples)
        xyz = DevicePool.synthetic(400 + N, B, N, 16, device=dev).data
        points = torch.from_numpy(np.ascontiguousarray(synth.normal(400 + N, 1, (B, N, D)))).to(dev) if D else None
        fps_idx = farthest_point_sample(xyz, S, torch.from_numpy(fps_start(1, B, N)).to(dev))
        new_xyz = torch.gather(xyz, 1, fps_idx.unsqueeze(2).expand(-1, -1, 3)).contiguous()
        _, c_r2, c_ns, _ = Gr._scales("time_msg", radii, nsamples)
        r2s = [Gr._r2(r) for r in radii]
        idx_cat = torch.empty(B, S, Ktot, dtype=torch.int64, device=dev)
        count_cat = torch.empty(B, S, R, dtype=torch.int32, device=dev)
        idxs = [torch.empty(B, S, k, dtype=torch.int64, device=dev) for k in nsamples]
        counts = [torch.empty(B, S, dtype=torch.int32, device=dev) for _ in nsamples]
        outs_msg = [torch.empty(B, S, k, D + 3, dtype=torch.float32, device=dev) for k in nsamples]
        outs_one = [torch.empty(B, S, k, 3 + D, dtype=torch.float32, device=dev) for k in nsamples]

        def query_msg():
            Gr._query_msg_launch(xyz, new_xyz, B, N, S, R, c_r2, c_ns, idx_cat, count_cat)

        def query_calls():
            for r2, k, idx, count in zip(r2s, nsamples, idxs, counts):
                Gr._query_launch(xyz, new_xyz, B, N, S, r2, k, idx, count)

        def group_msg():
            Gr._group_msg_launch(xyz, new_xyz, points, idx_cat, B, N, S, R, c_ns, nsamples, D, outs=outs_msg)

        def group_calls():
            for k, idx, out in zip(nsamples, idxs, outs_one):
                Gr._group_launch(xyz, new_xyz, points, idx, B, N, S, k, D, out)

        legs = [("query_msg", query_msg), ("query_calls", query_calls), ("group_msg", group_msg), ("group_calls", group_calls)]
        if D:
            dgs_msg = [torch.from_numpy(np.ascontiguousarray(synth.normal(500 + N, 2 + i, (B, S, k, D + 3)))).to(dev) for i, k in enumerate(nsamples)]
            dgs_one = [torch.cat([g[..., D:], g[..., :D]], dim=-1).contiguous() for g in dgs_msg]      # the same gradients, [xyz | attributes]
            d_msg = torch.empty(B, N, D, dtype=torch.float32, device=dev)
            d_one = [torch.empty(B, N, D, dtype=torch.float32, device=dev) for _ in nsamples]

            def bwd_msg():
                return Gr.group_points_msg_backward(dgs_msg, idx_cat, nsamples, N, out=d_msg)

            def bwd_calls():
                for g, idx, out in zip(dgs_one, idxs, d_one):
                    Gr.group_points_backward(g, idx, N, out=out)
                total = d_one[0] + d_one[1]
                for d in d_one[2:]:
                    total += d
                return total

            legs += [("bwd_msg", bwd_msg), ("bwd_calls", bwd_calls)]
        for _, fn in legs:
            fn()
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in legs}
        last = {}
        for _ in range(args.reps):
            for name, fn in legs:
                t, last[name] = timed(torch, fn, args.inner)
                res[name].append(t)
        med = {k: median(v) for k, v in res.items()}
        tag = "B %d N %d S %d r %s nsample %s D %d" % (B, N, S, "/".join("%g" % r for r in radii), "/".join("%d" % k for k in nsamples), D)
        labels = [("query_msg", "svnet_ball_query_msg_f32, one pass          "), ("query_calls", "%d x svnet_ball_query_f32                    " % R),
                  ("group_msg", "svnet_group_points_msg_f32, one launch      "), ("group_calls", "%d x svnet_group_points_f32                  " % R)]
        if D:
            labels += [("bwd_msg", "group_points_msg_backward (lists + sum)     "), ("bwd_calls", "%d x group_points_backward + %d adds          " % (R, R - 1))]
        for name, label in labels:
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[name], " ".join("%.3f" % v for v in res[name])))
        idx_diff = int((idx_cat != torch.cat(idxs, dim=2)).sum()) + int((count_cat != torch.stack(counts, dim=2)).sum())
        out_diff = sum(int((torch.cat([o[..., 3:], o[..., :3]], dim=-1).contiguous().view(torch.int32) != m.view(torch.int32)).sum())
                       for o, m in zip(outs_one, outs_msg))
        ratios = "query %.2f x;  group %.2f x" % (med["query_calls"] / med["query_msg"], med["group_calls"] / med["group_msg"])
        if D:
            diff = float((last["bwd_msg"] - last["bwd_calls"]).abs().max())
            ratios += ";  backward %.2f x (largest difference %.2e of %.1f)" % (med["bwd_calls"] / med["bwd_msg"], diff, float(last["bwd_msg"].abs().max()))
        else:
            ratios += ";  no backward at D = 0"
        lines.append("%s  R calls / one call: %s;  differing indices and counts %d, differing output words %d" % (tag, ratios, idx_diff, out_diff))
        seen = []
        for i, k in enumerate(nsamples):
            c, tail = counts[i].to(torch.int64), idxs[i][:, :, k - 1]
            seen.append(torch.where(c >= k, torch.clamp((tail // 64 + 1) * 64, max=N), torch.full_like(tail, N)))
        union = torch.stack(seen).max(dim=0)[0]
        lines.append("%s  scanned fraction of N per scale: %s (sum %.3f);  union, what the one pass scans: %.3f;  full groups per scale: %s %%"
                     % (tag, " ".join("%.3f" % (float(s.float().mean()) / N) for s in seen), sum(float(s.float().mean()) / N for s in seen),
                        float(union.float().mean()) / N,
                        " ".join("%.1f" % (100.0 * float((counts[i] >= k).float().mean())) for i, k in enumerate(nsamples))))
        del xyz, points, new_xyz, idx_cat, idxs, outs_msg, outs_one
        if D:
            del dgs_msg, dgs_one, d_msg, d_one
        last.clear()
        torch.cuda.empty_cache()
    emit(lines, args.out)


if __name__ == "__main__":
    main()
