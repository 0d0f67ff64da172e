"""Times of the fused set-abstraction level on the GPU (svnet_amd/sa_fused.py, csrc/sa_fused.hip) against the module's own eval
forward, HIP events around repeated calls, at

    (B 32, N 1024, S 512, r 0.2, nsample 32, D 0, widths 64/64/128)          the first level of a PointNet++ SSG classifier
    (B 32, N 512, S 128, r 0.4, nsample 64, D 128, widths 128/128/256)       its second level
    (B 32, N 1024, S 512, r 0.1/0.2/0.4, nsample 16/32/128, D 0, widths 32/32/64, 64/64/128, 64/96/128)    the first MSG level

on DevicePool.synthetic clouds with seeded parameters and running statistics away from identity.  Three legs per shape:

  1. FusedSetAbstraction(module)(xyz, points, start): sampling, centre gather, one query pass, one fused launch per scale;
  2. module(xyz, points, start) in eval mode under no_grad: the same sampling and query, the grouping, then torch's Conv2d +
     BatchNorm2d + ReLU stack and max - the yardstick, in the same process on the same machine;
  3. the fused launches alone, on the indices and counts of leg 1, into a buffer allocated before the clock starts.

Legs alternate after a warm-up of each shape; the median of the rounds is reported with every round listed.  Per shape the tool also
gives the output words of leg 1 that differ from leg 2 by more than tests/common.compare_case's measure allows at 1e-3 (|a - b| >
1e-3 max|b|; 0 expected) with the largest such ratio, the fraction of the group slots the kernel skips through `count`, and the fused
launches' rate as a fraction of the 155 TFLOP/s the f32-input MFMA sustains - from the products of the rows it really multiplies,
2 sum C_(l-1) C_l each, padding not counted.

    python tools/time_sa_fused.py [--out profiles/sa_fused_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

MFMA_F32_TFLOPS = 155.0
SHAPES = (("ssg1", 32, 1024, 512, (0.2,), (32,), 0, ((64, 64, 128),)),
          ("ssg2", 32, 512, 128, (0.4,), (64,), 128, ((128, 128, 256),)),
          ("msg1", 32, 1024, 512, (0.1, 0.2, 0.4), (16, 32, 128), 0, ((32, 32, 64), (64, 64, 128), (64, 96, 128))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_sa_fused.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import sa_fused as SF
    from svnet_amd import synth
    from svnet_amd.data import DevicePool, fps_start
    from svnet_amd.models.utils.pointnet_msg import PointNetSetAbstractionMsg
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for name, B, N, S, radii, nsamples, D, mlps in SHAPES:
        torch.manual_seed(600 + N)
        if len(radii) == 1:
            mod = PointNetSetAbstraction(S, radii[0], nsamples[0], D + 3, list(mlps[0]), False)
        else:
            mod = PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlps])
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                torch.nn.init.uniform_(m.weight, 0.5, 1.5)
                torch.nn.init.uniform_(m.bias, -0.5, 0.5)
                torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
                torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
        mod = mod.to(dev).eval()
        fused = SF.FusedSetAbstraction(mod)
        assert fused.supported(N, D)
        rows = DevicePool.synthetic(600 + N, B, N, 16, device=dev).data                       # [B,N,3]
        xyz = rows.permute(0, 2, 1).contiguous()
        points = torch.from_numpy(np.ascontiguousarray(synth.normal(600 + N, 1, (B, D, N)))).to(dev) if D else None
        attrs = None if points is None else points.permute(0, 2, 1).contiguous()
        start = torch.from_numpy(fps_start(1, B, N)).to(dev)

        # the indices and counts leg 3 runs on: the wrapper's own chain up to the query
        from svnet_amd import _pointset
        from svnet_amd.group import _query_msg_launch, _scales
        R, c_r2, c_ns, _ = _scales("time_sa_fused", radii, nsamples)
        Ktot, C = sum(nsamples), fused.channels
        fps_idx = torch.empty(B, S, dtype=torch.int64, device=dev)
        _pointset.fps_launch(rows, B, N, S, start, fps_idx)
        new_xyz = _pointset.gather_rows(rows, fps_idx).contiguous()
        idx = torch.empty(B, S, Ktot, dtype=torch.int64, device=dev)
        count = torch.empty(B, S, R, dtype=torch.int32, device=dev)
        _query_msg_launch(rows, new_xyz, B, N, S, R, c_r2, c_ns, idx, count)
        out = torch.empty(B, C, S, dtype=torch.float32, device=dev)

        def leg_fused():
            return fused(xyz, points, start=start)[1]

        def leg_module():
            with torch.no_grad():
                return mod(xyz, points, start=start)[1]

        def leg_kernel():
            off = c_off = 0
            for i, (level, k) in enumerate(zip(fused.levels, nsamples)):
                SF._launch(rows, new_xyz, idx[:, :, off:], Ktot, attrs, level, count[:, :, i:], R, fused.xyz_last, out, c_off, B, N, S, k, D)
                off += k
                c_off += level.widths[-1]
            return out

        legs = [("fused", leg_fused), ("module", leg_module), ("kernel", leg_kernel)]
        for _, fn in legs:
            fn()
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k, _ in legs}
        last = {}
        for _ in range(args.reps):
            for k, fn in legs:
                t, last[k] = timed(torch, fn, args.inner)
                res[k].append(t)
        med = {k: median(v) for k, v in res.items()}
        tag = "%s B %d N %d S %d r %s nsample %s D %d widths %s" % (name, B, N, S, "/".join("%g" % r for r in radii),
                                                                   "/".join("%d" % k for k in nsamples), D, " ".join("/".join(map(str, m)) for m in mlps))
        for k, label in (("fused", "FusedSetAbstraction, whole call        "), ("module", "module eval forward, whole call        "),
                         ("kernel", "%d x svnet_sa_fused_f32 alone           " % R)):
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))
        a, b = last["fused"].double(), last["module"].double()
        scale = float(b.abs().max())
        ratio = (a - b).abs() / scale
        same = int((last["kernel"].view(torch.int32) != last["fused"].view(torch.int32)).sum())
        kept = count.clamp(min=1).to(torch.int64)
        rows_done = [int(torch.minimum(kept[:, :, i], torch.tensor(k, device=dev)).sum()) for i, k in enumerate(nsamples)]
        flops = sum(2.0 * r * sum(ci * co for ci, co in zip((D + 3,) + tuple(m[:-1]), m)) for r, m in zip(rows_done, mlps))
        skipped = 1.0 - sum(rows_done) / float(B * S * Ktot)
        lines.append("%s  module / fused: %.2f x whole call;  words off by more than 1e-3 of the largest output: %d of %d (largest %.2e);  "
                     "kernel-alone words that differ from the whole call's: %d" % (tag, med["module"] / med["fused"], int((ratio > 1e-3).sum()),
                                                                                  ratio.numel(), float(ratio.max()), same))
        lines.append("%s  slots skipped through count: %.1f %%;  fused launches: %.2f GFLOP in %.3f ms = %.1f TFLOP/s, %.1f %% of %g"
                     % (tag, 100.0 * skipped, flops / 1e9, med["kernel"], flops / med["kernel"] / 1e9, 100.0 * flops / med["kernel"] / 1e9 / MFMA_F32_TFLOPS,
                        MFMA_F32_TFLOPS))
        del mod, fused, rows, xyz, points, attrs, idx, count, out
        last.clear()
        torch.cuda.empty_cache()
    emit(lines, args.out)


if __name__ == "__main__":
    main()
