"""Times of the distillation loss on the GPU (svnet_amd.train.kd_loss / kd_seg_loss / Distiller, csrc/loss.hip):

  rows   kd_loss forward + backward at (R, C) = (32, 40), beside cal_loss at the same shape;
  seg    kd_seg_loss forward + backward at (B, C, N) = (32, 50, 2048), beside seg_loss forward + backward at the same shape;
  loop   the flagship training loop (sv_dgcnn_cls --binary, B = 32, N = 1024, k = 20: captured step + captured FlatAdam) without a
         teacher, and (loop_kd) with a captured full-precision teacher in front of every step, and the teacher's forward alone.

"forward + backward" of a loss is what a train step pays between the model's forward and its backward: the loss call, and the gradient
of the logits as the model's last layer receives it - contiguous in the logits' layout, seeded with the step's cached unit gradient
(torch.autograd.grad(loss, logits, UNIT_GRAD) followed by .contiguous(): a no-op for the KD losses and cal_loss, the transposed
gradient copy for seg_loss).  Each pair is timed twice: launched eagerly (host-bound at these sizes: the number of launches counts)
and captured into a HIP graph and replayed (device time).  Legs alternate; medians of --reps windows.

Every leg runs in a child process of its own under `timeout`; the first leg that fails ends the run.

    python tools/time_kd.py [--out profiles/kd_times.txt] [--commit TEXT]
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

# (leg, its time limit in seconds).  The two loops are processes of their own: a captured FlatAdam re-packs the weights IT saw inside its
# graph, and a second student in the same process would send both optimizers down the eager re-pack.
LEGS = (("rows", 240), ("seg", 240), ("loop", 300), ("loop_kd", 300))


def _median(v):
    return sorted(v)[len(v) // 2]


def _window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls               # us per call


def _loss_pairs(torch, names_fns, reps, calls):
    """[(name, fn)] -> lines: eager and graph-replayed us per call, alternating legs."""
    graphs = {}
    for name, fn in names_fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
        graphs[name] = g
    res = {(name, mode): [] for name, _ in names_fns for mode in ("eager", "graph")}
    for _ in range(reps):
        for name, fn in names_fns:
            res[name, "eager"].append(_window(torch, fn, calls))
            res[name, "graph"].append(_window(torch, graphs[name].replay, calls))
    lines = []
    for name, _ in names_fns:
        for mode in ("eager", "graph"):
            v = res[name, mode]
            lines.append("  %-34s %-6s %9.2f us per call (median of %d windows of %d calls; %s)"
                         % (name, mode, _median(v), reps, calls, " ".join("%.2f" % x for x in v)))
    return lines, {k: _median(v) for k, v in res.items()}


def _fwd_bwd(torch, loss_of, logits):
    from svnet_amd import _ops
    unit = _ops.UNIT_GRAD.get(logits.device)

    def fn():
        (g,) = torch.autograd.grad(loss_of(logits), logits, unit)
        return g.contiguous()
    return fn


def leg_rows(torch, args):
    from svnet_amd.train import cal_loss, kd_loss
    dev = torch.device("cuda:0")
    R, C = 32, 40
    gen = torch.Generator().manual_seed(1)
    s = (torch.randn(R, C, generator=gen) * 3).to(dev).requires_grad_(True)
    t = (torch.randn(R, C, generator=gen) * 3).to(dev)
    y = torch.randint(0, C, (R,), generator=gen).to(dev)
    lines, _ = _loss_pairs(torch, [("kd_loss fwd+bwd (32, 40)", _fwd_bwd(torch, lambda x: kd_loss(x, t, y), s)),
                                   ("cal_loss fwd+bwd (32, 40)", _fwd_bwd(torch, lambda x: cal_loss(x, y), s))], args.reps, 200)
    return ["GPU %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__), "rows layout, (R, C) = (32, 40):"] + lines


def leg_seg(torch, args):
    from svnet_amd.train import kd_seg_loss, seg_loss
    dev = torch.device("cuda:0")
    B, C, N = 32, 50, 2048
    gen = torch.Generator().manual_seed(2)
    s = (torch.randn(B, C, N, generator=gen) * 3).to(dev).requires_grad_(True)
    t = (torch.randn(B, C, N, generator=gen) * 3).to(dev)
    y = torch.randint(0, C, (B, N), generator=gen).to(dev)
    kd_name, seg_name = "kd_seg_loss fwd+bwd (32, 50, 2048)", "seg_loss fwd+bwd (32, 50, 2048)"
    lines, med = _loss_pairs(torch, [(kd_name, _fwd_bwd(torch, lambda x: kd_seg_loss(x, t, y), s)),
                                     (seg_name, _fwd_bwd(torch, lambda x: seg_loss(x, y), s))], args.reps, 100)
    mb = B * C * N * 4 / 1e6
    lines.append("  bytes the algorithm needs: kd_seg_loss %.1f MB (two logit tensors in, one gradient out), seg_loss %.1f MB (logits, transposed "
                 "copy out and in, gradient out and in, transposed gradient out)" % (3 * mb, 6 * mb))
    lines.append("  kd_seg_loss, graph replay: %.2f TB/s of those bytes" % (3 * mb / med[kd_name, "graph"]))
    for mode in ("eager", "graph"):
        k, q = med[kd_name, mode], med[seg_name, mode]
        lines.append("  GATE (%s): kd_seg_loss %.2f us %s seg_loss %.2f us (%.2f x)" % (mode, k, "<=" if k <= q else ">  SLOWER THAN", q, q / k))
    return ["channel-major layout, (B, C, N) = (32, 50, 2048):"] + lines


def leg_loop(torch, args):
    import svnet_amd.models as M
    from svnet_amd import synth
    from svnet_amd.train import Distiller, FlatAdam, FlatParams, TrainStep
    dev = torch.device("cuda:0")
    B, N, k = 32, 1024, 20
    x = torch.from_numpy(synth.cloud_batch(1234, 0, 0, B, N)).to(dev)
    y = torch.from_numpy(synth.class_labels(1234, 0, 0, B)).to(dev)

    def model(binary):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            return M.SV_DGCNN_CLS(argparse.Namespace(k=k, binary=binary), 40).to(dev)

    def setup(with_teacher):
        student = model(True).train()
        flat = FlatParams(student)
        d = None
        if with_teacher:
            d = Distiller(model(False), (x,), T=4.0, alpha=0.5).capture()
            d.run()
        step = TrainStep(student, (x,), y, **({"loss_fn": d.loss_fn} if d else {})).capture()
        opt = FlatAdam(flat, step.bucket, lr=1e-3)

        def one():
            if d is not None:
                d.run()
            step.run(all_reduce=False)
            opt.step()
        for _ in range(3):
            one()
        opt.capture()
        for _ in range(3):
            one()
        return one, d, step

    def loop(one, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    one, d, step = setup(args.leg == "loop_kd")
    res = {"loop": [], "teacher": []}
    for _ in range(args.reps):
        res["loop"].append(loop(one, args.steps))
        if d is not None:
            res["teacher"].append(loop(d.run, args.steps))
    what = "sv_dgcnn_cls --binary, B = 32, N = 1024, k = 20 (captured step + captured FlatAdam; host clock around %d steps)" % args.steps
    if d is None:
        return ["flagship loop, %s:" % what,
                "  %-44s %8.3f ms per step (median of %d; %s)" % ("student alone", _median(res["loop"]), args.reps, " ".join("%.3f" % v for v in res["loop"]))]
    parts = [float(v) for v in d.parts]
    lines = ["flagship loop with a teacher, %s:" % what]
    for key, label in (("loop", "full-precision teacher (captured) + student"), ("teacher", "the teacher's forward alone")):
        lines.append("  %-44s %8.3f ms per step (median of %d; %s)" % (label, _median(res[key]), args.reps, " ".join("%.3f" % v for v in res[key])))
    lines.append("  {L, CE, KL} after the last step: %.4f %.4f %.4f" % tuple(parts))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to print as the commit (a tree that is no git checkout cannot tell)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--leg", choices=[l for l, _ in LEGS], default=None, help="run ONE leg in this process (what the driver starts)")
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("time_kd.py measures on the GPU: no HIP device here")
        lines = {"rows": leg_rows, "seg": leg_seg, "loop": leg_loop, "loop_kd": leg_loop}[args.leg](torch, args)
        print("\n".join(lines))
        return
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    text = ["commit %s" % (commit or "(not a git checkout)")]
    failed = None
    for leg, limit in LEGS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps),
               "--steps", str(args.steps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(res.stdout, end="", flush=True)
        if res.returncode != 0:
            failed = "leg %s FAILED with exit status %d: nothing after it was run" % (leg, res.returncode)
            text.append(res.stdout[-4000:])
            text.append(failed)
            break
        text.append(res.stdout.rstrip("\n"))
    out = "\n".join(text) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out)
    if failed:
        sys.exit(failed)


if __name__ == "__main__":
    main()
