#!/usr/bin/env python3
"""Generate tests/golden/msg.npz: the REFERENCE's multi-scale grouping level on small lattice inputs, recorded once.

    SVNET_REFERENCE=<checkout of the reference> python -m tests.golden.make_msg_golden          (from the repo root, CPU)

For every case of tests/msg_ref.GOLDEN_CASES - radii (0.125, 0.25, 0.5) with nsample (4, 8, 16) and D = 0, radii (0.1, 0.2, 0.4) with
nsample (8, 16, 32) and D = 4, both B = 2, N = 256, S = 32 - it runs models/utils/pointnet_util.py of the reference and stores data
only, no reference source:
  - the inputs "<name>_xyz" [B,N,3], "<name>_points" [B,N,D] (D > 0), the start "<name>_start" [B] that torch.randint draws first under
    torch.manual_seed(seed), and the loss weights "<name>_lw";
  - the centres "<name>_new_xyz" [B,S,3], the reference's `query_ball_point` per scale "<name>_idx<i>" [B,S,nsample_i], and the grouped
    tensors built with its helpers in the Msg order (forward, lines 248-255: index_points of the attributes, then the centred
    coordinates) "<name>_grouped<i>" [B,S,nsample_i,D+3];
  - `PointNetSetAbstractionMsg(S, radii, nsamples, D, mlp_list)`: the seeded state_dict "<name>_sd:<key>" (BatchNorm weights, biases
    and running statistics away from their identity start) with its keys and shapes "<name>_keys" / "<name>_shapes", and for
    <mode> = "ev" (eval: the running statistics of the state_dict normalise) and "tr" (train: batch statistics) the outputs
    "<name>_<mode>_out:new_xyz", "<name>_<mode>_out:new_points", the loss sum(new_points lw) "<name>_<mode>_out:loss", the parameter
    gradients "<name>_<mode>_d:<key>" and the gradient of the attributes "<name>_<mode>_dx:points" [B,D,N] (D > 0).  In train mode
    the gradients of the convolutions' biases are NOT recorded: a bias in front of batch statistics has a gradient of exactly zero
    (the generator asserts the float64 run gives less than 1e-9), and what fp32 computes there is rounding noise of the layers
    behind it - with D = 0 the first layer sees coordinates inside a small ball, mostly the zeros of padded slots, and the
    reference's own fp32 run misses its float64 run by 5e-3 of the case's largest gradient.  Eval mode records every gradient.
Coordinates are integer multiples of 2^-10 in [-1, 1), where the reference's expanded distance form is exact and equals the contract's
difference form; every centre is a point of its cloud.  While writing it asserts
  - the restatement (tests/fps_ref.fps_batch for the sampling, tests/msg_ref for the rest) reproduces the reference's centres, indices
    and grouped tensors bit for bit,
  - no recorded group is empty, and EVERY scale has at least one full group (cut at nsample) and one partial one (padded),
  - for the radii whose square is exact in fp32 every scale has a recorded group with a point at distance exactly r2 (inside); for
    the others r2 is no multiple of 2^-20 and no distance equals it,
  - on everything recorded, the reference's fp32 run and its float64 run agree within 1e-4 under tests.common.compare_case - a tenth
    of the tolerance the tests use, so no ReLU kink or max-pool tie sits on a knife edge; if they do not, pick another seed.
No test imports the reference: they read the .npz only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from svnet_amd import synth                   # noqa: E402
from tests import fps_ref as F                # noqa: E402
from tests import group_ref as G              # noqa: E402
from tests import msg_ref as M                # noqa: E402
from tests.common import compare_case         # noqa: E402


def ref_module(name, rel):
    ref = os.environ.get("SVNET_REFERENCE")
    if not ref:
        sys.exit("set SVNET_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run_module(U, name, state, x, pts, lw, dtype, train):
    """The reference's module in `dtype` -> {key: numpy float64}: outputs, loss, parameter gradients, attribute gradient."""
    seed, B, N, S, radii, nsamples, D, mlp_list = M.GOLDEN_CASES[name]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                      # the reference's sampling builds its distance table in the default dtype
    try:
        mod = U.PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlp_list])
        mod.load_state_dict(state, strict=True)
        mod.to(dtype).train(train)
        tx = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dtype)
        tp = None if pts is None else torch.from_numpy(np.ascontiguousarray(pts.transpose(0, 2, 1))).to(dtype).requires_grad_()
        torch.manual_seed(seed)
        new_xyz, new_points = mod(tx, tp)
        loss = (new_points * torch.from_numpy(lw).to(dtype)).sum()
        loss.backward()
        res = {"out:new_xyz": new_xyz.detach().numpy().astype(np.float64), "out:new_points": new_points.detach().numpy().astype(np.float64),
               "out:loss": np.array([float(loss.detach())])}
        if tp is not None:
            res["dx:points"] = tp.grad.numpy().astype(np.float64)
        for k, p in mod.named_parameters():
            res["d:" + k] = p.grad.numpy().astype(np.float64)
        return res
    finally:
        torch.set_default_dtype(old)


def main():
    U = ref_module("ref_pointnet_util", os.path.join("models", "utils", "pointnet_util.py"))
    out = {}
    for name, (seed, B, N, S, radii, nsamples, D, mlp_list) in M.GOLDEN_CASES.items():
        R = len(radii)
        torch.manual_seed(seed)
        start = torch.randint(0, N, (B,), dtype=torch.long).numpy().astype(np.int64)     # the sampling's first draw under this seed
        x, pts = M.golden_inputs(name, start)
        assert x.shape == (B, N, 3) and np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -1 and x.max() < 1
        tx, tp = torch.from_numpy(x), None if pts is None else torch.from_numpy(pts)

        # ---- the helpers: sampling, centres, the query per scale, the grouped tensors in the Msg order
        torch.manual_seed(seed)
        with torch.no_grad():
            fps_idx = U.farthest_point_sample(tx, S)
            new_xyz = U.index_points(tx, fps_idx)
            idxs, grouped = [], []
            for radius, k in zip(radii, nsamples):
                idx = U.query_ball_point(radius, k, tx, new_xyz)
                gx = U.index_points(tx, idx) - new_xyz.view(B, S, 1, 3)
                grouped.append(gx if tp is None else torch.cat([U.index_points(tp, idx), gx], dim=-1))
                idxs.append(idx)
        fps_idx = fps_idx.numpy().astype(np.int64)
        new_xyz = np.ascontiguousarray(new_xyz.numpy())
        idxs = [i.numpy().astype(np.int64) for i in idxs]
        grouped = [np.ascontiguousarray(g.numpy()) for g in grouped]
        assert np.array_equal(fps_idx[:, 0], start), "%s: the sampling did not start where torch.randint was expected to point" % name
        assert np.array_equal(F.fps_batch(x, S, start), fps_idx), "%s: the sampling restatement differs from the reference" % name
        assert np.array_equal(_bits(new_xyz), _bits(np.stack([x[b, fps_idx[b]] for b in range(B)])))

        r2s = [G.r2_of(r) for r in radii]
        idx_cat, count = M.query_ball_msg_batch(x, new_xyz, r2s, nsamples)
        assert idx_cat.shape == (B, S, sum(nsamples)) and count.shape == (B, S, R)
        assert np.array_equal(idx_cat, np.concatenate(idxs, axis=2)), "%s: the restatement's indices differ from the reference's" % name
        assert (count >= 1).all(), "%s: an empty group" % name
        mine = M.group_msg_batch(x, new_xyz, idx_cat, nsamples, pts)
        exact = all(r in G.EXACT_RADII for r in radii)
        for i in range(R):
            assert grouped[i].shape == (B, S, nsamples[i], D + 3) and grouped[i].dtype == np.float32
            assert np.array_equal(_bits(mine[i]), _bits(grouped[i])), "%s: grouped tensor %d differs" % (name, i)
            full, partial = int((count[..., i] == nsamples[i]).sum()), int((count[..., i] < nsamples[i]).sum())
            assert full >= 1 and partial >= 1, "%s scale %d: %d full and %d partial groups - change the seed or the shape" % (name, i, full, partial)
            on_sphere = sum(int((np.take_along_axis(G.distances(new_xyz[b], x[b]), idxs[i][b], axis=1) == r2s[i]).any(axis=1).sum()) for b in range(B))
            if exact:
                assert float(r2s[i]) == radii[i] * radii[i] and on_sphere >= 1, "%s scale %d: no group holds a point at distance exactly r2" % (name, i)
            else:
                assert float(r2s[i]) * 2 ** 20 != round(float(r2s[i]) * 2 ** 20) and on_sphere == 0
            print("  %-5s scale %d radius %-5g nsample %2d  counts %2d..%2d, %2d of %2d groups full, %d hold a point on the sphere"
                  % (name, i, radii[i], nsamples[i], count[..., i].min(), count[..., i].max(), full, count[..., i].size, on_sphere))

        # ---- the module
        mlp_out = sum(m[-1] for m in mlp_list)
        lw = synth.normal(seed, 5, (B, mlp_out, S))
        torch.manual_seed(seed)
        mod = U.PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlp_list])
        for bns in mod.bn_blocks:                           # BatchNorm away from its identity start
            for bn in bns:
                torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
                torch.nn.init.uniform_(bn.bias, -0.5, 0.5)
                torch.nn.init.uniform_(bn.running_mean, -0.25, 0.25)
                torch.nn.init.uniform_(bn.running_var, 0.5, 1.5)
        state = {k: v.clone() for k, v in mod.state_dict().items()}
        assert any(k.startswith("conv_blocks.%d.1." % (R - 1)) for k in state) and any(k.startswith("bn_blocks.0.0.") for k in state)
        runs = {}
        for mode, train in (("ev", False), ("tr", True)):
            r32, r64 = (_run_module(U, name, {k: v.clone() for k, v in state.items()}, x, pts, lw, dt, train) for dt in (torch.float32, torch.float64))
            if train:
                for k in [k for k in r32 if k.startswith("d:conv_blocks.") and k.endswith(".bias")]:
                    assert np.abs(r64[k]).max() < 1e-9, "%s: %s is not a zero gradient" % (name, k)
                    del r32[k], r64[k]
            worst = compare_case(r32, r64, 1e-4, "%s %s fp32 against float64" % (name, mode))
            print("  %-5s module, %s: fp32 against float64 worst %.3e at %s" % ((name, mode) + worst))
            assert np.array_equal(_bits(r32["out:new_xyz"].transpose(0, 2, 1)), _bits(new_xyz)), "%s: the module sampled other centres" % name
            runs[mode] = r32

        out[name + "_xyz"], out[name + "_start"], out[name + "_new_xyz"], out[name + "_lw"] = x, start, new_xyz, lw
        if pts is not None:
            out[name + "_points"] = pts
        for i in range(R):
            out["%s_idx%d" % (name, i)], out["%s_grouped%d" % (name, i)] = idxs[i].astype(np.int16), grouped[i]
        for k, v in state.items():
            out["%s_sd:%s" % (name, k)] = v.numpy()
        for mode, res in runs.items():
            for k, v in res.items():
                out["%s_%s_%s" % (name, mode, k)] = v.astype(np.float32)
        out[name + "_keys"] = np.array(list(state))
        out[name + "_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in state.values()], dtype=np.int64)
    path = os.path.join(HERE, "msg.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
