"""Times of the fused feature-propagation level on the GPU (svnet_amd/fp_fused.py, csrc/fp_fused.hip) against the module's own eval
forward, HIP events around repeated calls, at the three decoder levels of a PointNet++ part-segmentation model, B 32:

    (N 2048, S 512, D1 22, D2 128, widths 128/128/128)       the last level: the dense cloud, 16 labels + xyz twice as skip features
    (N 512, S 128, D1 128, D2 256, widths 256/128)           the middle level
    (N 128, S 1, D1 256, D2 1024, widths 256/256)            the first level, behind the group_all abstraction: the `S == 1` branch

on DevicePool.synthetic clouds - the sampled points are the first S of the N dense ones, so every sampled point coincides with a dense
one, as after farthest point sampling - with seeded parameters and running statistics away from identity.  Three legs per shape:

  1. FusedFeaturePropagation(module)(xyz1, xyz2, points1, points2): three_nn, then one fused launch;
  2. module(xyz1, xyz2, points1, points2) in eval mode under no_grad: the same three_nn, three_interpolate, torch.cat, then torch's
     Conv1d + BatchNorm1d + ReLU stack - the yardstick, in the same process on the same machine;
  3. the fused launch alone, on the indices and weights of leg 1, into a buffer allocated before the clock starts.

Legs alternate after a warm-up of each shape; the median of the rounds is reported with every round listed.  Per shape the tool also
gives the output words of leg 1 that differ from leg 2 by more than tests/common.compare_case's measure allows at 1e-3 (|a - b| >
1e-3 max|b|; 0 expected) with the largest such ratio, the points per workgroup of the plan, and the fused launch's rate as a fraction
of the 155 TFLOP/s the f32-input MFMA sustains (tools/microbench) - from the products of the rows it really multiplies,
2 sum C_(l-1) C_l each, padding not counted.

    python tools/time_fp_fused.py [--out profiles/fp_fused_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

MFMA_F32_TFLOPS = 155.0
SHAPES = (("fp1", 32, 2048, 512, 22, 128, (128, 128, 128)),
          ("fp2", 32, 512, 128, 128, 256, (256, 128)),
          ("fp3", 32, 128, 1, 256, 1024, (256, 256)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_fp_fused.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import fp_fused as FP
    from svnet_amd import propagate, synth
    from svnet_amd.data import DevicePool
    from svnet_amd.models.utils.pointnet_util import PointNetFeaturePropagation
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for name, B, N, S, D1, D2, widths in SHAPES:
        torch.manual_seed(700 + N)
        mod = PointNetFeaturePropagation(D1 + D2, list(widths))
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                torch.nn.init.uniform_(m.weight, 0.5, 1.5)
                torch.nn.init.uniform_(m.bias, -0.5, 0.5)
                torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
                torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
        mod = mod.to(dev).eval()
        fused = FP.FusedFeaturePropagation(mod)
        assert fused.supported(N, S, D1, D2)
        rows1 = DevicePool.synthetic(700 + N, B, N, 16, device=dev).data                      # [B,N,3]
        rows2 = rows1[:, :S].contiguous()
        xyz1, xyz2 = rows1.permute(0, 2, 1).contiguous(), rows2.permute(0, 2, 1).contiguous()
        points1 = torch.from_numpy(np.ascontiguousarray(synth.normal(700 + N, 1, (B, D1, N)))).to(dev)
        points2 = torch.from_numpy(np.ascontiguousarray(synth.normal(700 + N, 2, (B, D2, S)))).to(dev)
        idx, _, weight = propagate.three_nn(rows1, rows2)                                     # what leg 3 runs on
        out = torch.empty(B, widths[-1], N, dtype=torch.float32, device=dev)

        def leg_fused():
            return fused(xyz1, xyz2, points1, points2)

        def leg_module():
            with torch.no_grad():
                return mod(xyz1, xyz2, points1, points2)

        def leg_kernel():
            FP._launch(idx, weight, points2, points1, fused.level, out, 0, B, N, S, D1, D2)
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
        tag = "%s B %d N %d S %d D1 %d D2 %d widths %s" % (name, B, N, S, D1, D2, "/".join(map(str, widths)))
        for k, label in (("fused", "FusedFeaturePropagation, whole call    "), ("module", "module eval forward, whole call        "),
                         ("kernel", "svnet_fp_fused_f32 alone               ")):
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))
        a, b = last["fused"].double(), last["module"].double()
        ratio = (a - b).abs() / float(b.abs().max())
        same = int((last["kernel"].view(torch.int32) != last["fused"].view(torch.int32)).sum())
        flops = 2.0 * B * N * sum(ci * co for ci, co in zip((D1 + D2,) + tuple(widths[:-1]), widths))
        lines.append("%s  module / fused: %.2f x whole call;  words off by more than 1e-3 of the largest output: %d of %d (largest %.2e);  "
                     "kernel-alone words that differ from the whole call's: %d" % (tag, med["module"] / med["fused"], int((ratio > 1e-3).sum()),
                                                                                  ratio.numel(), float(ratio.max()), same))
        lines.append("%s  %d points per workgroup;  fused launch: %.2f GFLOP in %.3f ms = %.1f TFLOP/s, %.1f %% of %g"
                     % (tag, FP.rows_tile(D1, D2, widths), flops / 1e9, med["kernel"], flops / med["kernel"] / 1e9,
                        100.0 * flops / med["kernel"] / 1e9 / MFMA_F32_TFLOPS, MFMA_F32_TFLOPS))
        del mod, fused, rows1, rows2, xyz1, xyz2, points1, points2, idx, weight, out
        last.clear()
        torch.cuda.empty_cache()
    emit(lines, args.out)


if __name__ == "__main__":
    main()
