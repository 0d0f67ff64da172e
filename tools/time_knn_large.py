"""Times knn() past the register-resident range (DESIGN.md "Streamed k-NN"): HIP events around each call after warm-up, B = 8,
N in {4096, 4160, 8192, 16384, 32768} x C in {3, 62, 127} x k in {20, 40, 128}.  C = 3 is the coordinate graph ([B,3,N] contiguous),
the others the feature graphs (transposed views of [B,N,C]).  N = 4096 at k <= 64 is the register-resident kernel: the yardstick.

Prints per shape: us per call (median of --iters), ns per (query, candidate) pair (B N^2 pairs), the per-pair cost relative to N = 4096
at the same C and k ("vs4096"), and at k = 128 also relative to the register-resident kernel at N = 4096, k = 40 ("vs_reg").
Run on the GPU: python tools/time_knn_large.py [--iters 10] > knn_large_times.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=8)
    a = ap.parse_args()
    from svnet_amd.models.utils.sv_util import knn
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    B = a.B
    per_pair = {}
    print("%6s %4s %4s %11s %9s %7s %7s" % ("N", "C", "k", "us/call", "ns/pair", "vs4096", "vs_reg"))
    for C in (3, 62, 127):
        for k in (20, 40, 128):
            for N in (4096, 4160, 8192, 16384, 32768):
                if C == 3:
                    x = torch.randn(B, C, N, generator=g).to(dev)
                else:
                    x = torch.randn(B, N, C, generator=g).to(dev).transpose(-1, -2)
                for _ in range(a.warmup):
                    knn(x, k)
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    knn(x, k)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                us = sorted(ts)[len(ts) // 2]
                ns = us * 1e3 / (B * N * N)
                per_pair[(N, C, k)] = ns
                rel = ns / per_pair[(4096, C, k)]
                reg = ("%7.2f" % (ns / per_pair[(4096, C, 40)])) if k > 64 else "      -"
                print("%6d %4d %4d %11.1f %9.4f %7.2f %s" % (N, C, k, us, ns, rel, reg), flush=True)
                del x


if __name__ == "__main__":
    main()
