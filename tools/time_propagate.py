"""Times of the feature propagation on the GPU (svnet_amd/propagate.py, csrc/propagate.hip), HIP events around repeated launches:

  1. svnet_three_nn_f32, svnet_three_interpolate_f32 and the two in sequence (Propagator.run: fixed buffers) and propagate() (what a
     caller pays: + the three allocations) at (B, P, N, D) = (32, 10000, 2048, 50) and (32, 10000, 1024, 50) - a part-segmentation
     batch of 10 000-point clouds sampled down to 2048 / 1024 points;
  2. at the same shapes, the reference's formula (models/utils/pointnet_util.py:281-308) restated with torch operations on the device:
     what a user has without the kernels.  Written here from the contract in svnet_amd/propagate.py's docstring: the difference-form
     distance matrix [B,P,N], topk(3, largest=False), reciprocal weights, gather and weighted sum.  It runs at the largest batch that
     fits (halved on an out-of-memory error, the time scaled to B clouds) and is a timing yardstick, not a bit-exact twin (topk may
     order ties differently); the tool prints how far its output is from the kernels';
  3. train.evaluate_dense against train.evaluate per batch (M 64 clouds of 10 000 points sampled to 2048, batch 32, 50 parts) with a
     stand-in forward step (one small einsum), so the difference is the propagation plus the metrics launch over P instead of N points.

Legs alternate inside this one process after a warm-up of each shape.  The `out` write of the interpolation (B D P 4 bytes) over its
time is reported as a fraction of the 8 TB/s HBM peak.

    python tools/time_propagate.py [--out profiles/propagate_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

SHAPES = ((32, 10000, 2048, 50), (32, 10000, 1024, 50))
HBM_PEAK = 8.0e12


def torch_ops_propagate(torch, q, r, f):
    """[B,P,3], [B,N,3], [B,D,N] -> [B,D,P] with torch operations only."""
    d = q[:, :, None, 0] - r[:, None, :, 0]
    dist = d * d
    d = q[:, :, None, 1] - r[:, None, :, 1]
    dist += d * d
    d = q[:, :, None, 2] - r[:, None, :, 2]
    dist += d * d
    del d
    dist3, idx = dist.topk(min(3, r.shape[1]), dim=2, largest=False)
    del dist
    rec = 1.0 / (dist3 + 1e-8)
    w = rec / rec.sum(dim=2, keepdim=True)
    B, D, N = f.shape
    P, K = idx.shape[1], idx.shape[2]
    g = torch.gather(f, 2, idx.reshape(B, 1, P * K).expand(B, D, P * K)).view(B, D, P, K)
    return (g * w[:, None]).sum(dim=3)


class StandIn:
    """The ForwardStep protocol without a model: logits [B,50,N] = a fixed affine function of loader.x."""

    def __init__(self, torch, loader, parts):
        self.torch, self.loader = torch, loader
        g = torch.Generator(device="cpu").manual_seed(5)
        self.W = torch.randn(parts, 3, generator=g).to(loader.x.device)
        self.out = None

    def run(self):
        self.out = self.torch.einsum("cd,bdn->bcn", self.W, self.loader.x).contiguous()
        return self.out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_propagate.py measures on the GPU: no HIP device here")
    import numpy as np
    from svnet_amd import synth
    from svnet_amd import propagate as Pr
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    from svnet_amd.train import evaluate, evaluate_dense
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)" % (args.inner, args.reps))
    for B, P, N, D in SHAPES:
        q = torch.from_numpy(np.ascontiguousarray(synth.normal(300 + N, 0, (B, P, 3)))).to(dev)
        r = q[:, :N].contiguous()                          # the sampled points coincide with dense points, as after resample_fps
        f = torch.from_numpy(np.ascontiguousarray(synth.normal(300 + N, 1, (B, D, N)))).to(dev)
        prop = Pr.Propagator(B, D, N, P, dev)

        def nn():
            Pr._nn_launch(q, r, B, P, N, prop.idx, prop.dist3, prop.weight)

        def interp():
            Pr._interp_launch(f, prop.idx, prop.weight, B, D, N, P, prop.out)

        def both():
            return prop.run(q, r, f)

        def public():
            return Pr.propagate(q, r, f)

        tb = B
        while True:                                        # the largest batch the torch restatement fits
            try:
                torch_ops_propagate(torch, q[:tb], r[:tb], f[:tb])
                torch.cuda.synchronize()
                break
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
                if tb == 1:
                    raise
                tb //= 2

        def ops():
            return torch_ops_propagate(torch, q[:tb], r[:tb], f[:tb])

        legs = (("nn", nn, args.inner), ("interp", interp, args.inner), ("both", both, args.inner), ("public", public, args.inner),
                ("ops", ops, 2))
        for _, fn, _ in legs:
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _, _ in legs}
        for _ in range(args.reps):
            for name, fn, inner in legs:
                t, out = timed(torch, fn, inner)
                res[name].append(t * (B / tb if name == "ops" else 1.0))
                if name == "both":
                    mine = out.clone()
                elif name == "ops":
                    diff = float((out - mine[:tb]).abs().max())
        med = {k: median(v) for k, v in res.items()}
        tag = "B %d P %d N %d D %d" % (B, P, N, D)
        labels = (("nn", "svnet_three_nn_f32              "), ("interp", "svnet_three_interpolate_f32     "),
                  ("both", "Propagator.run (both, fixed buf)"), ("public", "propagate() (+ 3 allocations)   "),
                  ("ops", "torch ops, batch %2d, scaled     " % tb))
        for name, label in labels:
            lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[name], " ".join("%.3f" % v for v in res[name])))
        out_bytes = B * D * P * 4
        lines.append("%s  torch ops / propagate() = %.1f x;  / Propagator.run = %.1f x;  max |torch ops - kernels| = %.2e"
                     % (tag, med["ops"] / med["public"], med["ops"] / med["both"], diff))
        lines.append("%s  %.2f G distance pairs: %.0f G pairs/s;  out write %.1f MB: %.2f TB/s = %.2f of the 8 TB/s HBM peak (interpolate alone)"
                     % (tag, B * P * N / 1e9, B * P * N / 1e9 / (med["nn"] * 1e-3), out_bytes / 1e6, out_bytes / (med["interp"] * 1e-3) / 1e12,
                        out_bytes / (med["interp"] * 1e-3) / HBM_PEAK))
        del q, r, f, prop
        torch.cuda.empty_cache()

    # evaluate_dense against evaluate, per batch
    M, P, N, Bt, parts = 64, 10000, 2048, 32, 50
    dense = DevicePool.synthetic(7, M, P, 16, parts, device=dev)
    pool = dense.resample_fps(N, seed=1, normalize=True)
    loader = BatchLoader(pool, Bt, N, select="first_ordered", scale_shift=False, rotate="none", shuffle=False, drop_last=False, seed=1)
    step = StandIn(torch, loader, parts)
    metrics = EpochMetrics(parts, dev, parts=SHAPENET_PARTS, capacity=M)
    res = {"evaluate": [], "evaluate_dense": []}
    evaluate(step, loader, metrics)                        # warm-up of both passes
    evaluate_dense(step, loader, metrics, dense)
    for _ in range(args.reps):
        for name, fn in (("evaluate", lambda: evaluate(step, loader, metrics)),
                         ("evaluate_dense", lambda: evaluate_dense(step, loader, metrics, dense))):
            t, out = timed(torch, fn, 1)
            res[name].append(t / len(loader))
            if name == "evaluate_dense":
                dense_iou = out["shape_iou"]
            else:
                sample_iou = out["shape_iou"]
    tag = "M %d P %d N %d batch %d, stand-in forward" % (M, P, N, Bt)
    for name in ("evaluate", "evaluate_dense"):
        lines.append("%s  %-15s %9.3f ms per batch  (%s)" % (tag, name, median(res[name]), " ".join("%.3f" % v for v in res[name])))
    lines.append("%s  (the pass includes its one host read and, for evaluate_dense, source_points and the buffer allocation;  shape IoU of the "
                 "sample %.4f, of the clouds %.4f)" % (tag, sample_iou, dense_iou))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
