"""Times of the device-resident loader (svnet_amd/data.py, csrc/batch.hip) on the GPU:

  1. the assembly launch alone (HIP events around `reps` back-to-back launches) at (B, P, N) = (32, 2048, 1024) and (32, 2048, 2048)
     for each select mode, with scale/shift + SO(3) rotation;
  2. a train_epoch-style loop of sv_dgcnn_cls --binary (B 32, N 1024, k 20: bench.py's flagship step, captured, FlatAdam captured)
     over a synthetic pool, WITH `loader.load(i)` in front of every step against the same loop WITHOUT it (fixed buffers: what the
     step benchmark does).  Both legs run in this one process on the same captured graphs, alternating, `rounds` times each.

    python tools/time_loader.py [--out profiles/loader_times.txt]
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


def launch_alone(torch, dev, lines, reps=200):
    from svnet_amd.data import BatchLoader, DevicePool
    pool = DevicePool.synthetic(11, 256, 2048, 40, 50, device=dev)
    for N in (1024, 2048):
        for select in ("first_shuffled", "subset", "first_ordered"):
            ld = BatchLoader(pool, 32, N, select=select, scale_shift=True, rotate="so3", seed=1, num_cat=16)
            for i in range(8):
                ld.load(i % len(ld))
            torch.cuda.synchronize()
            best = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(reps):
                    ld.load(i % len(ld))
                b.record()
                torch.cuda.synchronize()
                best.append(a.elapsed_time(b) / reps * 1e3)
            lines.append("launch alone  B 32 P 2048 N %4d %-14s  %7.2f us per launch (median of 5 x %d back-to-back; min %.2f max %.2f)"
                         % (N, select, sorted(best)[2], reps, min(best), max(best)))


def train_loop(torch, dev, lines, steps, rounds):
    import svnet_amd.models as M
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.train import FlatAdam, FlatParams, TrainStep
    B, N, k = 32, 1024, 20
    pool = DevicePool.synthetic(12, 1024, 2048, 40, device=dev)
    ld = BatchLoader(pool, B, N, select="first_shuffled", scale_shift=True, rotate="none", seed=1)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = M.SV_DGCNN_CLS(argparse.Namespace(k=k, binary=True, dropout=0.5), 40).to(dev).train()
    flat = FlatParams(model)
    ld.load(0)
    step = TrainStep(model, (ld.x,), ld.y).capture()
    step.run(all_reduce=False)
    opt = FlatAdam(flat, step.bucket, lr=1e-3)
    opt.capture()

    def loop(n, with_load):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            if with_load:
                ld.load(i % len(ld))
            step.run(all_reduce=False)
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
    for leg, name in ((False, "fixed buffers (no load)"), (True, "with loader.load(i)    ")):
        lines.append("train loop    sv_dgcnn_cls --binary B 32 N 1024 k 20, %s  %.3f ms per step (median of %d x %d steps; %s)"
                     % (name, med[leg], rounds, steps, " ".join("%.3f" % v for v in res[leg])))
    lines.append("train loop    loader cost %+.3f ms per step = %+.2f %% of the fixed-buffer loop"
                 % (med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_loader.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    lines = []
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?")
    lines.append("commit %s   GPU %s   CPU %s   torch %s" % (commit or "(not a git checkout)", torch.cuda.get_device_name(0), cpu, torch.__version__))
    launch_alone(torch, dev, lines)
    train_loop(torch, dev, lines, args.steps, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
