"""Times of the fused global set-abstraction level on the GPU (svnet_amd/sa_global.py, csrc/sa_global.hip) against the module's own
eval forward, HIP events around repeated calls, at

    (B 32, N 128, D 256, widths 256/512/1024)        the third level of a PointNet++ SSG classifier
    (B 32, N 128, D 640, widths 256/512/1024)        the third level of the MSG classifier

with seeded parameters and running statistics away from identity.  Three legs per shape:

  1. FusedGlobalAbstraction(module)(xyz, points): the two launches and the allocation of the results;
  2. module(xyz, points) in eval mode under no_grad: the row-major copies, the concatenation, torch's Conv2d + BatchNorm2d + ReLU stack
     and max - the yardstick, in the same process on the same machine;
  3. svnet_sa_global_f32 alone - its two launches - into a buffer allocated before the clock starts.

Then the three-level SSG encoder at B 32, N 1024 - FusedSetAbstraction on (512, 0.2, 32, 64/64/128) and (128, 0.4, 64, 128/128/256),
FusedGlobalAbstraction on the global level - against the three modules in eval mode, eager and as a captured graph (device starts).

Legs alternate after a warm-up of each shape; the median of the rounds is reported with every round listed.  Per shape the tool also
gives the largest difference of leg 1 from leg 2 relative to the largest output (tests/common.compare_case's measure) and the
launches' rate as a fraction of the 155 TFLOP/s the f32-input MFMA sustains - from the products of the rows it really multiplies,
2 sum C_(l-1) C_l each, padding not counted.  A ratio below 1 is marked LOSS.

    python tools/time_sa_global.py [--out profiles/sa_global_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

MFMA_F32_TFLOPS = 155.0
SHAPES = (("ssg3", 32, 128, 256, (256, 512, 1024)), ("msg3", 32, 128, 640, (256, 512, 1024)))
ENCODER = (32, 1024, ((512, 0.2, 32, (64, 64, 128)), (128, 0.4, 64, (128, 128, 256))), (256, 512, 1024))


def _seed_bns(torch, mod):
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
            torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
            torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
    return mod


def _rounds(torch, legs, reps, inner):
    for _, fn in legs:
        fn()
        fn()
    torch.cuda.synchronize()
    res, last = {k: [] for k, _ in legs}, {}
    for _ in range(reps):
        for k, fn in legs:
            t, last[k] = timed(torch, fn, inner)
            res[k].append(t)
    return res, {k: median(v) for k, v in res.items()}, last


def _verdict(ratio):
    return "%.2f x%s" % (ratio, "  LOSS" if ratio < 1.0 else "")


def _worst(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _captured(torch, dev, fn):
    """fn captured into a graph on a side stream after a warm-up there -> (replay, the captured result)."""
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = fn()

    def replay():
        graph.replay()
        return res
    return replay, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_sa_global.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import sa_fused as SF
    from svnet_amd import sa_global as SG
    from svnet_amd import synth
    from svnet_amd.data import DevicePool, fps_start
    from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for name, B, N, D, mlp in SHAPES:
        torch.manual_seed(700 + D)
        mod = _seed_bns(torch, PointNetSetAbstraction(None, None, None, D + 3, list(mlp), True)).to(dev).eval()
        fused = SG.FusedGlobalAbstraction(mod)
        assert fused.supported(N, D)
        xyz = DevicePool.synthetic(700 + D, B, N, 16, device=dev).data.permute(0, 2, 1).contiguous()              # [B,3,N]
        points = torch.from_numpy(np.ascontiguousarray(synth.normal(700 + D, 1, (B, D, N)))).to(dev)
        out = torch.empty(B, mlp[-1], 1, dtype=torch.float32, device=dev)

        def leg_fused():
            return fused(xyz, points)[1]

        def leg_module():
            with torch.no_grad():
                return mod(xyz, points)[1]

        def leg_kernel():
            SG._launch(xyz, points, fused.level, out, 0, B, N, D)
            return out

        res, med, last = _rounds(torch, [("fused", leg_fused), ("module", leg_module), ("kernel", leg_kernel)], args.reps, args.inner)
        tag = "%s B %d N %d D %d widths %s" % (name, B, N, D, "/".join(map(str, mlp)))
        for k, label in (("fused", "FusedGlobalAbstraction, whole call     "), ("module", "module eval forward, whole call        "),
                         ("kernel", "svnet_sa_global_f32 alone (2 launches) ")):
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))
        same = int((last["kernel"].view(torch.int32) != last["fused"].view(torch.int32)).sum())
        flops = 2.0 * B * N * sum(ci * co for ci, co in zip((D + 3,) + tuple(mlp[:-1]), mlp))
        lines.append("%s  module / fused: %s whole call;  worst difference from the module relative to the largest output: %.2e;  "
                     "kernel-alone words that differ from the whole call's: %d" % (tag, _verdict(med["module"] / med["fused"]),
                                                                                  _worst(last["fused"], last["module"]), same))
        lines.append("%s  %d points per workgroup, %d workgroups;  launches: %.2f GFLOP in %.3f ms = %.1f TFLOP/s, %.1f %% of %g"
                     % (tag, SG.rows_tile(D, mlp), B * -(-N // SG.rows_tile(D, mlp)), flops / 1e9, med["kernel"], flops / med["kernel"] / 1e9,
                        100.0 * flops / med["kernel"] / 1e9 / MFMA_F32_TFLOPS, MFMA_F32_TFLOPS))
        del mod, fused, xyz, points, out
        last.clear()
        torch.cuda.empty_cache()

    # ---- the three-level SSG encoder
    B, N, local, mlp3 = ENCODER
    torch.manual_seed(777)
    mods, last_c = [], 0
    for S, radius, nsample, mlp in local:
        mods.append(_seed_bns(torch, PointNetSetAbstraction(S, radius, nsample, last_c + 3, list(mlp), False)).to(dev).eval())
        last_c = mlp[-1]
    mods.append(_seed_bns(torch, PointNetSetAbstraction(None, None, None, last_c + 3, list(mlp3), True)).to(dev).eval())
    fuseds = [SF.FusedSetAbstraction(m) for m in mods[:-1]] + [SG.FusedGlobalAbstraction(mods[-1])]
    xyz = DevicePool.synthetic(777, B, N, 16, device=dev).data.permute(0, 2, 1).contiguous()
    starts, n = [], N
    for S, _, _, _ in local:
        starts.append(torch.from_numpy(fps_start(1, B, n)).to(dev))
        n = S
    starts.append(None)

    def chain(levels):
        def run():
            with torch.no_grad():
                x, p = xyz, None
                for level, start in zip(levels, starts):
                    x, p = level(x, p, start=start)
                return p
        return run

    tag = "ssg encoder B %d N %d  %s, global %s" % (B, N, "  ".join("(%d, %g, %d, %s)" % (S, r, k, "/".join(map(str, m))) for S, r, k, m in local),
                                                     "/".join(map(str, mlp3)))
    res, med, last = _rounds(torch, [("fused", chain(fuseds)), ("module", chain(mods))], args.reps, args.inner)
    for k, label in (("fused", "three fused levels, eager              "), ("module", "three modules in eval mode, eager      ")):
        lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))
    lines.append("%s  modules / fused, eager: %s;  worst difference from the modules relative to the largest output: %.2e"
                 % (tag, _verdict(med["module"] / med["fused"]), _worst(last["fused"], last["module"])))
    try:
        replay_f, gf = _captured(torch, dev, chain(fuseds))
        replay_m, gm = _captured(torch, dev, chain(mods))
    except Exception as e:                                  # a module that cannot be captured: reported, not hidden
        lines.append("%s  captured graphs: not measured (%s: %s)" % (tag, type(e).__name__, str(e).splitlines()[0][:120]))
    else:
        res, med, last = _rounds(torch, [("fused", replay_f), ("module", replay_m)], args.reps, args.inner)
        for k, label in (("fused", "three fused levels, captured graph     "), ("module", "three modules in eval mode, captured   ")):
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))
        lines.append("%s  modules / fused, captured: %s;  worst difference from the modules relative to the largest output: %.2e"
                     % (tag, _verdict(med["module"] / med["fused"]), _worst(last["fused"], last["module"])))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
