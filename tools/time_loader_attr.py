"""Times of the per-point attributes on the device data path (svnet_amd/data.py, csrc/batch.hip, csrc/fps.hip) on the GPU, by the method
of tools/time_loader.py (HIP events around `reps` back-to-back launches, median of 5):

  1. the assembly launch alone at (B 32, P 2048, N 1024, first_shuffled, scale/shift + SO(3)) for A = 0, A = 3 with one normal, A = 6
     with two normals and A = 9 scalars; for A > 0 the attribute traffic (B N A floats read as rows, the same written as planes) over
     the time the launch takes beyond the A = 0 launch;
  2. the A = 0 launch of this tree's library against another build of it (--parent path/to/libsvnet_hip.so, the parent commit's:
     make -C svnet_amd/csrc BUILD=_build_parent OUT=../../_ab/libparent.so in a checkout of the parent): one child process per run,
     alternating, --runs times each.  The child binds the library it is given with ctypes itself (a library of another ABI number
     is what this leg is for; the descriptor's attribute fields stay zero, which an older library never reads).  Unchanged = the
     median of this tree's medians is not above the parent's by more than the parent's own spread;
  3. DevicePool.resample_fps (M 64, P 10000 -> 1024) with A = 6 and without.

    python tools/time_loader_attr.py [--parent _ab/libparent.so] [--runs 3] [--out profiles/loader_attr_times.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(B=32, P=2048, N=1024, M=256)
ATTRS = [(0, 0), (3, 1), (6, 2), (9, 0)]


def _attr(M, P, A, k, seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, P, A))
    for j in range(k):
        a[:, :, 3 * j:3 * j + 3] /= np.sqrt((a[:, :, 3 * j:3 * j + 3] ** 2).sum(-1, keepdims=True))
    return a.astype(np.float32)


def _median_us(torch, launch, reps):
    for i in range(8):
        launch(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            launch(i)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps * 1e3)
    return sorted(times)[2], min(times), max(times)


def launch_alone(torch, dev, lines, reps=200):
    from svnet_amd.data import BatchLoader, DevicePool
    B, P, N, M = (SHAPE[k] for k in "BPNM")
    data, label, _ = DevicePool.synthetic_arrays(11, M, P, 40)
    base = None
    for A, k in ATTRS:
        pool = DevicePool(data, label, attr=_attr(M, P, A, k) if A else None, attr_vectors=k, device=dev)
        ld = BatchLoader(pool, B, N, select="first_shuffled", scale_shift=True, rotate="so3", seed=1)
        med, lo, hi = _median_us(torch, lambda i: ld.load(i % len(ld)), reps)
        text = "launch alone  B %d P %d N %d first_shuffled scale_shift so3  A %d (%d normals)  %7.2f us per launch (median of 5 x %d; min %.2f max %.2f)" \
               % (B, P, N, A, k, med, reps, lo, hi)
        if A == 0:
            base = med
        else:
            traffic = 2.0 * B * N * A * 4
            extra = med - base
            text += "  attributes: %.0f KB in + out, %+.2f us over A 0" % (traffic / 1e3, extra)
            text += " = %.1f GB/s" % (traffic / (extra * 1e-6) / 1e9) if extra > 0 else " (within the noise of the A 0 launch)"
        lines.append(text)


def child(lib_path, reps=200):
    """One run of leg 2: the A = 0 launch through the library at `lib_path`, bound here; prints the median in us."""
    import torch
    from svnet_amd import _lib
    from svnet_amd.data import DevicePool, epoch_order
    dev = torch.device("cuda:0")
    B, P, N, M = (SHAPE[k] for k in "BPNM")
    L = ctypes.CDLL(lib_path)
    L.svnet_batch_assemble_f32.restype = ctypes.c_int
    L.svnet_batch_assemble_f32.argtypes = [ctypes.POINTER(_lib.BatchDesc), ctypes.c_void_p]
    L.svnet_version.restype = ctypes.c_int
    data, label, _ = DevicePool.synthetic_arrays(11, M, P, 40)
    t = dict(data=torch.from_numpy(data).to(dev), label=torch.from_numpy(label).to(dev),
             order=torch.from_numpy(epoch_order(1, 0, M)).to(dev), x=torch.zeros(B, 3, N, device=dev),
             y=torch.zeros(B, dtype=torch.int64, device=dev), params=torch.zeros(B, 16, device=dev))
    d = _lib.BatchDesc()                                    # zero-filled: no seg, no one-hot, no attributes
    for name, v in t.items():
        setattr(d, name, v.data_ptr())
    d.M, d.P, d.L, d.B, d.N, d.count, d.seed, d.epoch = M, P, M, B, N, B, 1, 0
    d.select_mode, d.scale_shift, d.rotate = 0, 1, 2
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    steps = M // B

    def launch(i):
        d.first = (i % steps) * B
        if L.svnet_batch_assemble_f32(ctypes.byref(d), stream) != 0:
            sys.exit("svnet_batch_assemble_f32 failed in %s" % lib_path)
    med, lo, hi = _median_us(torch, launch, reps)
    if not bool(torch.isfinite(t["x"]).all()):
        sys.exit("non-finite x from %s" % lib_path)
    print("CHILD %d %.3f %.3f %.3f" % (L.svnet_version(), med, lo, hi))


def against_parent(lines, parent, runs):
    from svnet_amd import _lib
    libs = [("parent", os.path.abspath(parent)), ("this", _lib.LIB_PATH)]
    res, abi = {n: [] for n, _ in libs}, {}
    for _ in range(runs):
        for name, path in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], capture_output=True, text=True, timeout=300)
            row = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("CHILD ")]
            if out.returncode != 0 or not row:          # nothing more is started on a GPU that may have faulted
                sys.exit("%s: the child ended with %d: %s" % (name, out.returncode, (out.stderr or out.stdout)[-800:]))
            abi[name] = int(row[-1][1])
            res[name].append(float(row[-1][2]))
    med = {n: statistics.median(v) for n, v in res.items()}
    spread = max(res["parent"]) - min(res["parent"])
    for name, _ in libs:
        lines.append("A 0 launch    %-6s library (ABI %d)  %7.3f us (median of %d runs' medians; runs %s; spread %.3f)"
                     % (name, abi[name], med[name], runs, " ".join("%.3f" % v for v in res[name]), max(res[name]) - min(res[name])))
    lines.append("A 0 launch    this - parent = %+.3f us, parent's spread %.3f us: %s"
                 % (med["this"] - med["parent"], spread, "unchanged" if med["this"] - med["parent"] <= spread else "SLOWER"))


def resample(torch, dev, lines):
    import numpy as np
    from svnet_amd.data import DevicePool
    M, P, N, A = 64, 10000, 1024, 6
    rng = np.random.default_rng(2)
    data, label = rng.standard_normal((M, P, 3)).astype(np.float32), rng.integers(0, 40, M)
    for with_attr in (False, True):
        pool = DevicePool(data, label, attr=_attr(M, P, A, 1) if with_attr else None, attr_vectors=int(with_attr), device=dev)
        med, lo, hi = _median_us(torch, lambda i: pool.resample_fps(N, seed=0, normalize=True), 3)
        lines.append("resample_fps  M %d P %d -> %d  A %d  %9.1f us per call (median of 5 x 3; min %.1f max %.1f)"
                     % (M, P, N, A if with_attr else 0, med, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="the parent commit's libsvnet_hip.so (leg 2; skipped without it)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    lines = []
    if args.parent:                                         # first: the children run while this process has not opened the GPU
        against_parent(lines, args.parent, args.runs)
    else:
        lines.append("A 0 launch    against the parent's library: not run (no --parent)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_loader_attr.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    head = "commit %s   GPU %s   torch %s" % (commit or "(not a git checkout)", torch.cuda.get_device_name(0), torch.__version__)
    launch_alone(torch, dev, lines)
    resample(torch, dev, lines)
    text = "\n".join([head] + lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
