"""Times of the epoch metrics (svnet_amd/metrics.py, csrc/metrics.hip) on the GPU:

  1. the update call alone (HIP events around `reps` back-to-back updates) at classification B 32, C 40 and at part segmentation
     B 32, 50 parts x 2048 points;
  2. a train_epoch-style loop of sv_dgcnn_cls --binary (B 32, N 1024, k 20: bench.py's flagship step, captured with keep_output=True,
     FlatAdam captured, loader.load(i) in front of every step) WITH `metrics.update` behind every step against the same loop WITHOUT
     it.  Both legs run in this one process on the same captured graphs, alternating, `rounds` times each.

    python tools/time_metrics.py [--out profiles/metrics_times.txt]
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(torch, fn, reps):
    best = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / reps * 1e3)
    return sorted(best)[2], min(best), max(best)


def update_alone(torch, dev, lines, reps=200):
    from svnet_amd.metrics import SHAPENET_PARTS, EpochMetrics
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(32, 40, device=dev, generator=g)
    y = torch.randint(0, 40, (32,), device=dev, generator=g)
    m = EpochMetrics(40, dev)
    xs = torch.randn(32, 50, 2048, device=dev, generator=g)
    lab = torch.randint(0, 16, (32,), device=dev, generator=g)
    seg = torch.randint(0, 50, (32, 2048), device=dev, generator=g)
    ms = EpochMetrics(50, dev, parts=SHAPENET_PARTS, capacity=32)
    legs = (("cls B 32 C 40              ", lambda: m.update(x, y), x.numel() * 4),
            ("seg B 32 parts 50 N 2048   ", lambda: ms.update(xs, seg, label=lab), xs.numel() * 4 + seg.numel() * 8))
    for name, fn, nbytes in legs:
        for _ in range(8):
            fn()
        torch.cuda.synchronize()
        med, lo, hi = _events(torch, fn, reps)
        lines.append("update alone  %s %7.2f us per update (median of 5 x %d back-to-back; min %.2f max %.2f); %.1f MB read = %.2f TB/s"
                     % (name, med, reps, lo, hi, nbytes / 1e6, nbytes / med / 1e6))


def train_loop(torch, dev, lines, steps, rounds):
    import svnet_amd.models as M
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.metrics import EpochMetrics
    from svnet_amd.train import FlatAdam, FlatParams, TrainStep
    B, N, k = 32, 1024, 20
    pool = DevicePool.synthetic(12, 1024, 2048, 40, device=dev)
    ld = BatchLoader(pool, B, N, select="first_shuffled", scale_shift=True, rotate="none", seed=1)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = M.SV_DGCNN_CLS(argparse.Namespace(k=k, binary=True, dropout=0.5), 40).to(dev).train()
    flat = FlatParams(model)
    ld.load(0)
    step = TrainStep(model, (ld.x,), ld.y, keep_output=True).capture()
    step.run(all_reduce=False)
    opt = FlatAdam(flat, step.bucket, lr=1e-3)
    opt.capture()
    metrics = EpochMetrics(40, dev)

    def loop(n, with_metrics):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            ld.load(i % len(ld))
            step.run(all_reduce=False)
            if with_metrics:
                metrics.update(step.out, ld.y, B)
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    loop(5, True)
    loop(5, False)
    res = {True: [], False: []}
    for _ in range(rounds):
        for leg in (False, True):
            res[leg].append(loop(steps, leg))
    med = {leg: sorted(v)[len(v) // 2] for leg, v in res.items()}
    for leg, name in ((False, "without metrics       "), (True, "with metrics.update   ")):
        lines.append("train loop    sv_dgcnn_cls --binary B 32 N 1024 k 20, %s  %.3f ms per step (median of %d x %d steps; %s)"
                     % (name, med[leg], rounds, steps, " ".join("%.3f" % v for v in res[leg])))
    lines.append("train loop    metrics cost %+.3f ms per step = %+.2f %% of the loop without metrics"
                 % (med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False]))
    r = metrics.result()
    lines.append("train loop    the epoch's state after %d updates: rows %d, invalid %d, loss %.4f, acc %.4f"
                 % (r["rows"] // B, r["rows"], r["invalid"], r["loss"], r["acc"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_metrics.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    lines = []
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?")
    lines.append("commit %s   GPU %s   CPU %s   torch %s" % (commit or "(not a git checkout)", torch.cuda.get_device_name(0), cpu, torch.__version__))
    update_alone(torch, dev, lines)
    train_loop(torch, dev, lines, args.steps, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
