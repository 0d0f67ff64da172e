"""Times of the gradients of interpolation and grouping on the GPU (svnet_amd/csrc/pointset_grad.hip), HIP events around repeated
launches, by the method of tools/time_propagate.py:

  interpolation at (B, P, N, D) = (32, 10000, 2048, 50); grouping at (B, N, S, radius, nsample, D) = (32, 2048, 512, 0.4, 64, 64) and
  (32, 1024, 512, 0.2, 32, 64).  Per shape: the reverse-list build alone (svnet_pointset_reverse_i32), the sum kernel alone
  (svnet_three_interpolate_bwd_f32 / svnet_group_points_bwd_f32 on lists built once), the functional backward (both, + the
  allocations), and the backward pass of propagate() / group_points() through autograd (torch.autograd.grad on a retained graph);
  against the same gradient through torch operations: autograd of the forward restated with torch.gather (what tools/time_propagate.py
  and tools/time_group.py hold), whose backward scatters with float atomics.  The largest difference between the two gradients is
  printed; torch's depends on the arrival order of its atomics, the kernels' does not.

Every shape runs in a child process under its own time limit; inside it the legs alternate after a warm-up.

    python tools/time_pointset_grad.py [--out profiles/pointset_grad_times.txt]
"""
import argparse
import subprocess
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

INTERP_SHAPES = ((32, 10000, 2048, 50),)
GROUP_SHAPES = ((32, 2048, 512, 0.4, 64, 64), (32, 1024, 512, 0.2, 32, 64))
CHILD_LIMIT = 240          # seconds per shape


def _report(tag, legs, reps, torch, extra):
    for _, fn, _ in legs:
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in legs}
    for _ in range(reps):
        for name, fn, inner in legs:
            res[name].append(timed(torch, fn, inner)[0])
    med = {k: median(v) for k, v in res.items()}
    lines = ["%s  %-44s %9.3f ms  (%s)" % (tag, name, med[name], " ".join("%.3f" % v for v in res[name])) for name, _, _ in legs]
    lines.append("%s  torch autograd / .backward() here = %.2f x;  %s" % (tag, med["torch ops: autograd of the gather form"] / med[".backward() through autograd"], extra))
    return lines


def interp_child(shape, reps, inner):
    import numpy as np
    import torch
    from svnet_amd import _lib, _ops, _pointset, synth
    from svnet_amd import propagate as Pr
    B, P, N, D = shape
    dev = torch.device("cuda:0")
    q = torch.from_numpy(np.ascontiguousarray(synth.normal(300 + N, 0, (B, P, 3)))).to(dev)
    r = q[:, :N].contiguous()
    f = torch.from_numpy(np.ascontiguousarray(synth.normal(300 + N, 1, (B, D, N)))).to(dev)
    dout = torch.from_numpy(np.ascontiguousarray(synth.normal(300 + N, 2, (B, D, P)))).to(dev)
    idx, _, w = Pr.three_nn(q, r)
    rev_start, rev_edge = _pointset.reverse_lists(idx, N)
    dfeat = torch.empty(B, D, N, device=dev)
    leaf = f.clone().requires_grad_()
    mine_out = Pr.three_interpolate(leaf, idx, w)
    leaf_t = f.clone().requires_grad_()
    g = torch.gather(leaf_t, 2, idx.reshape(B, 1, P * 3).expand(B, D, P * 3)).view(B, D, P, 3)
    torch_out = (g * w[:, None]).sum(dim=3)

    def sums():
        _lib.call("svnet_three_interpolate_bwd_f32", _ops._p(dout), _ops._p(w), _ops._p(rev_start), _ops._p(rev_edge), B, D, N, P, _ops._p(dfeat),
                  _ops._stream())

    legs = (("svnet_pointset_reverse_i32", lambda: _pointset.reverse_lists(idx, N), inner),
            ("svnet_three_interpolate_bwd_f32", sums, inner),
            ("three_interpolate_backward() (both)", lambda: Pr.three_interpolate_backward(dout, idx, w, N), inner),
            (".backward() through autograd", lambda: torch.autograd.grad(mine_out, leaf, dout, retain_graph=True)[0], inner),
            ("torch ops: autograd of the gather form", lambda: torch.autograd.grad(torch_out, leaf_t, dout, retain_graph=True)[0], inner))
    a, b = legs[3][1](), legs[4][1]()
    lengths = (rev_start[:, 1:] - rev_start[:, :-1]).float()
    extra = "max |difference| %.2e of max |gradient| %.2e;  lists: mean %.1f, max %d edges" % (
        float((a - b).abs().max()), float(a.abs().max()), float(lengths.mean()), int(lengths.max()))
    return _report("interpolation B %d P %d N %d D %d" % shape, legs, reps, torch, extra)


def group_child(shape, reps, inner):
    import numpy as np
    import torch
    from svnet_amd import _lib, _ops, _pointset, synth
    from svnet_amd import group as Gr
    B, N, S, radius, nsample, D = shape
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(synth.uniform(400 + N, 0, (B, N, 3), -1.0, 1.0))).to(dev)
    pts = torch.from_numpy(np.ascontiguousarray(synth.normal(400 + N, 1, (B, N, D)))).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(synth.normal(400 + N, 2, (B, S, nsample, 3 + D)))).to(dev)
    new_xyz, _ = Gr.sample_and_group(S, radius, nsample, x, None)
    idx = Gr.query_ball_point(radius, nsample, x, new_xyz)
    rev_start, rev_edge = _pointset.reverse_lists(idx, N)
    dpoints = torch.empty(B, N, D, device=dev)
    leaf = pts.clone().requires_grad_()
    mine_out = Gr.group_points(x, new_xyz, idx, leaf)
    leaf_t = pts.clone().requires_grad_()
    flat = idx.view(B, S * nsample)
    centred = torch.gather(x, 1, flat.unsqueeze(2).expand(-1, -1, 3)).view(B, S, nsample, 3) - new_xyz[:, :, None]
    torch_out = torch.cat([centred, torch.gather(leaf_t, 1, flat.unsqueeze(2).expand(-1, -1, D)).view(B, S, nsample, D)], dim=3)

    def sums():
        _lib.call("svnet_group_points_bwd_f32", _ops._p(g), _ops._p(rev_start), _ops._p(rev_edge), B, N, S, nsample, D, _ops._p(dpoints),
                  _ops._stream())

    legs = (("svnet_pointset_reverse_i32", lambda: _pointset.reverse_lists(idx, N), inner),
            ("svnet_group_points_bwd_f32", sums, inner),
            ("group_points_backward() (both)", lambda: Gr.group_points_backward(g, idx, N), inner),
            (".backward() through autograd", lambda: torch.autograd.grad(mine_out, leaf, g, retain_graph=True)[0], inner),
            ("torch ops: autograd of the gather form", lambda: torch.autograd.grad(torch_out, leaf_t, g, retain_graph=True)[0], inner))
    a, b = legs[3][1](), legs[4][1]()
    lengths = (rev_start[:, 1:] - rev_start[:, :-1]).float()
    extra = "max |difference| %.2e of max |gradient| %.2e;  lists: mean %.1f, max %d edges" % (
        float((a - b).abs().max()), float(a.abs().max()), float(lengths.mean()), int(lengths.max()))
    return _report("grouping B %d N %d S %d radius %g nsample %d D %d" % shape, legs, reps, torch, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--child", default=None, help="internal: interp:<i> or group:<i>, one shape in this process")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_pointset_grad.py measures on the GPU: no HIP device here")
    if args.child:
        kind, i = args.child.split(":")
        fn, shapes = (interp_child, INTERP_SHAPES) if kind == "interp" else (group_child, GROUP_SHAPES)
        print("\n".join(fn(shapes[int(i)], args.reps, args.inner)))
        return
    lines = [header(torch)]
    lines.append("ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed); one child process per shape"
                 % (args.inner, args.reps))
    for child in ["interp:%d" % i for i in range(len(INTERP_SHAPES))] + ["group:%d" % i for i in range(len(GROUP_SHAPES))]:
        cmd = [sys.executable, __file__, "--child", child, "--reps", str(args.reps), "--inner", str(args.inner)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within %d s" % (child, CHILD_LIMIT))
            break                                                   # nothing more is started after a leg that hung
        if res.returncode != 0:
            lines.append("%s: exit status %d: %s" % (child, res.returncode, res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ""))
            break
        lines.extend(res.stdout.strip().splitlines())
    emit(lines, args.out)


if __name__ == "__main__":
    main()
