"""GPU tests (-m gpu) of the fused feature-propagation level: svnet_fp_fused_f32 (svnet_amd/csrc/fp_fused.hip) through
svnet_amd.fp_fused, against the numpy restatement tests/fp_fused_ref.py, the module's own eval forward and the reference's recorded
outputs (tests/golden/fp_fused.npz).  The contract is a fixed sequence of single-rounded operations and a fixed fmaf chain per output,
so the kernel's results are compared as BIT PATTERNS (a -0 counted as +0); the wrapper against the module, which rounds differently,
within the project's activation tolerance tests.common.compare_case(..., 1e-3).  Every case runs at B = 2; every reference is computed
once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import fp_fused_ref as R
from tests import fused_level_cases as FL
from tests import propagate_ref as P
from tests.common import compare_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B = 2
_once = FL.cache()

# (N, S, D1, D2, widths): every N in {1, 3, 63, 64, 65, 131} (a lone point, tile tails on both sides of one 64-point tile, three
# tiles; all but 64 no multiple of 4, so the last layer's scalar stores run, at 64 the 16-byte ones), every S in {1, 2, 3, 40} (empty
# neighbour slots), every (D1, D2) in {(0, 1), (3, 5), (6, 64), (0, 67), (131, 1)} (no skip features, K of the first product below,
# at and past one k-step, a multiple of nothing), one to four layers, widths that are no multiple of the 16-column tile, 196 and 256
# (more column tiles than waves).  The last two are the plans of 32 and 16 rows, at N 70: three and five tiles, the last partial.
CASES = [(1, 1, 0, 1, (5,)),
         (3, 2, 3, 5, (12, 20)),
         (63, 3, 6, 64, (33, 8, 196)),
         (64, 40, 0, 67, (16, 16, 16, 7)),
         (65, 40, 131, 1, (256,)),
         (131, 3, 3, 5, (33, 8, 196)),
         (64, 2, 6, 64, (256,)),
         (70, 40, 132, 256, (256, 128)),
         (70, 40, 512, 1024, (256, 256))]
ROWS = {(70, 40, 132, 256, (256, 128)): 32, (70, 40, 512, 1024, (256, 256)): 16}       # points per workgroup where they are not 64


def _inputs(N, S, D1, D2):
    """(idx [B,N,3], weight [B,N,3], points2 [B,D2,S], points1 [B,D1,N] or None): the neighbours and weights of the restated three_nn
    on Gaussian clouds, then two points' indices moved outside [0, S) - the kernel clamps them, the restatement too."""
    def make():
        q, r, f2 = P.gauss_case(7000 + N + S, B, N, S, D2)
        idx, _, w = P.three_nn_batch(q, r)
        idx = idx.copy()
        idx[:, 0, 0], idx[:, -1, 2] = -7, S + 3
        f1 = np.ascontiguousarray(synth.normal(7100 + N, D1, (B, D1, N))) if D1 else None
        return idx, np.ascontiguousarray(w), f2, f1
    return _once(("in", N, S, D1, D2), make)


def _want(N, S, D1, D2, widths):
    def make():
        idx, w, f2, f1 = _inputs(N, S, D1, D2)
        return R.level_batch(idx, w, f2, f1, FL.state(9100 + D1 + D2, D1 + D2, widths)[1])
    return _once(("want", N, S, D1, D2, widths), make)


@pytest.mark.parametrize("N,S,D1,D2,widths", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_level_equals_the_restatement_bit_for_bit(N, S, D1, D2, widths, hip_device):
    from svnet_amd import fp_fused as FP
    dev = hip_device
    assert FP.rows_tile(D1, D2, widths) == ROWS.get((N, S, D1, D2, widths), 64)
    idx, w, f2, f1 = _inputs(N, S, D1, D2)
    want = _want(N, S, D1, D2, widths)
    level, _ = FL.level(dev, 9100 + D1 + D2, D1 + D2, widths, conv_dim=1)
    tag = "N %d S %d D1 %d D2 %d widths %s" % (N, S, D1, D2, widths)
    ti, tw, t2, t1 = FL.dev(dev, idx, w, f2, f1)
    got = FP.interp_mlp(ti, tw, t2, t1, level)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, widths[-1], N) and got.is_contiguous()
    FL.same_bits(got, want, tag)
    assert float(want.max()) > 0
    # the clamp: the same indices clamped on the host give the same bits; a second run too
    FL.same_bits(FP.interp_mlp(ti.clamp(0, S - 1), tw, t2, t1, level), want, tag + ", clamped on the host")
    FL.same_bits(FP.interp_mlp(ti, tw, t2, t1, level), want, tag + ", again")
    # into channels 3 .. of a NaN-filled [B,C_total,N]: the other channels stay NaN
    C = widths[-1]
    buf = torch.full((B, C + 5, N), float("nan"), dtype=torch.float32, device=dev)
    assert FP.interp_mlp(ti, tw, t2, t1, level, out=buf, c_off=3) is buf
    FL.same_bits(buf[:, 3:3 + C].contiguous(), want, tag + ", c_off 3")
    assert torch.isnan(buf[:, :3]).all() and torch.isnan(buf[:, 3 + C:]).all()
    # one point on its own (B 1, N 1) has the bits it has inside a tile
    b, p = B - 1, N // 2
    alone = FP.interp_mlp(ti[b:b + 1, p:p + 1].contiguous(), tw[b:b + 1, p:p + 1].contiguous(), t2[b:b + 1],
                          None if t1 is None else t1[b:b + 1, :, p:p + 1].contiguous(), level)
    FL.same_bits(alone, want[b:b + 1, :, p:p + 1], tag + ", one point alone")


def test_interp_mlp_follows_three_nn_on_the_device(hip_device):
    """idx and weight straight from the device's three_nn, S below, at and above three: the restatement on the restated three_nn."""
    from svnet_amd import fp_fused as FP
    from svnet_amd import propagate as PR
    dev = hip_device
    for N, S, D1, D2, widths in [(65, 1, 0, 6, (8,)), (65, 2, 3, 5, (12, 20)), (131, 40, 6, 64, (33, 8, 196))]:
        def make():
            q, r, f2 = P.gauss_case(7300 + S, B, N, S, D2)
            f1 = np.ascontiguousarray(synth.normal(7300 + S, 9, (B, D1, N))) if D1 else None
            idx, _, w = P.three_nn_batch(q, r)
            return q, r, f2, f1, R.level_batch(idx, w, f2, f1, FL.state(7300 + S, D1 + D2, widths)[1])
        q, r, f2, f1, want = _once(("nn", N, S, D1, D2, widths), make)
        level, _ = FL.level(dev, 7300 + S, D1 + D2, widths, conv_dim=1)
        tq, tr, t2, t1 = FL.dev(dev, q, r, f2, f1)
        idx, _, weight = PR.three_nn(tq, tr)
        FL.same_bits(FP.interp_mlp(idx, weight, t2, t1, level), want, "S %d behind three_nn" % S)


# ---- the wrapper
def _golden_module(name, dev):
    """(module in eval mode on the device, xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] or None, points2 [B,D2,S], the recorded output)."""
    from svnet_amd.models.utils.pointnet_util import PointNetFeaturePropagation
    G = np.load(os.path.join(HERE, "golden", "fp_fused.npz"))
    seed, Bc, N, S, D1, D2, widths = R.GOLDEN_CASES[name]
    mod = PointNetFeaturePropagation(D1 + D2, list(widths))
    mod.load_state_dict({str(k): torch.from_numpy(G["%s_sd:%s" % (name, k)]) for k in G[name + "_keys"]}, strict=True)
    xyz1, xyz2, f1, f2 = FL.dev(dev, G[name + "_xyz1"].transpose(0, 2, 1), G[name + "_xyz2"].transpose(0, 2, 1), G[name + "_points1"] if D1 else None,
                              G[name + "_points2"])
    return mod.to(dev).eval(), xyz1, xyz2, f1, f2, G[name + "_ev_out"]


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_wrapper_equals_the_module_and_the_recorded_reference(name, hip_device):
    """FusedFeaturePropagation against the module's own eval forward on the same state_dict and against the reference's recorded
    eval output, both within compare_case(..., 1e-3), the project's activation tolerance (the composed path rounds the BatchNorm after
    the convolution, the fused one folds it in); and bit for bit against the restatement.  Then refresh()."""
    from svnet_amd import fp_fused as FP
    mod, xyz1, xyz2, f1, f2, ref = _golden_module(name, hip_device)
    fused = FP.FusedFeaturePropagation(mod)
    got = fused(xyz1, xyz2, f1, f2)
    with torch.no_grad():
        want = mod(xyz1, xyz2, f1, f2)
    assert got.dtype == torch.float32 and got.shape == want.shape and not got.requires_grad and got.is_contiguous()
    worst_mod = compare_case({"out:new_points": got.cpu().numpy()}, {"out:new_points": want.cpu().numpy()}, 1e-3, name + " against the module")
    worst_ref = compare_case({"out:new_points": got.cpu().numpy()}, {"out:new_points": ref}, 1e-3, name + " against the recorded reference")
    print("%s: worst relative error %.3e against the module, %.3e against the reference" % (name, worst_mod[0], worst_ref[0]))
    G = np.load(os.path.join(HERE, "golden", "fp_fused.npz"))
    FL.same_bits(got, _once(("golden", name), lambda: R.golden_restatement(G, name)), name + " against the restatement")
    # new running statistics: stale until refresh()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.add_(0.25)
        moved = mod(xyz1, xyz2, f1, f2)
    assert torch.equal(fused(xyz1, xyz2, f1, f2).view(torch.int32), got.view(torch.int32))
    fresh = fused.refresh()(xyz1, xyz2, f1, f2)
    compare_case({"out:new_points": fresh.cpu().numpy()}, {"out:new_points": moved.cpu().numpy()}, 1e-3, name + ", refreshed")
    assert not torch.equal(fresh, got)


def test_wrapper_refuses_train_mode_and_falls_back_outside_the_envelope(hip_device):
    from svnet_amd import fp_fused as FP
    from svnet_amd.models.utils.pointnet_util import PointNetFeaturePropagation
    dev = hip_device
    mod, xyz1, xyz2, f1, f2, _ = _golden_module("a", dev)
    fused = FP.FusedFeaturePropagation(mod)
    mod.train()
    with pytest.raises(RuntimeError, match="train mode"):
        fused(xyz1, xyz2, f1, f2)
    mod.eval()
    with pytest.raises(ValueError, match="points2 requires grad"):
        fused(xyz1, xyz2, f1, f2.clone().requires_grad_())
    # a layer of 300 channels is outside the kernel's limits: the module's own forward, bit for bit
    torch.manual_seed(5)
    wide = PointNetFeaturePropagation(12, [16, 300]).to(dev).eval()
    fused_wide = FP.FusedFeaturePropagation(wide)
    assert not fused_wide.supported(96, 24, 5, 7) and fused.supported(96, 24, 5, 7) and not fused.supported(96, 24, 5, 8)
    got = fused_wide(xyz1, xyz2, f1, f2)
    with torch.no_grad():
        want = wide(xyz1, xyz2, f1, f2)
    assert tuple(got.shape) == (B, 300, 96) and not got.requires_grad
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_wrapper_in_a_captured_graph(hip_device):
    """The wrapper captured on a side stream after a warm-up; two replays with the inputs refilled in place between them each give
    the eager result bit for bit."""
    from svnet_amd import fp_fused as FP
    from svnet_amd.models.utils.pointnet_util import PointNetFeaturePropagation
    dev = hip_device
    N, S, D1, D2 = 131, 40, 6, 10
    torch.manual_seed(9)
    mod = PointNetFeaturePropagation(D1 + D2, [12, 20]).to(dev).eval()
    fused = FP.FusedFeaturePropagation(mod)
    sets = []
    for seed in (90, 91):
        q, r, f2 = P.gauss_case(seed, B, N, S, D2)
        sets.append(FL.dev(dev, q.transpose(0, 2, 1), r.transpose(0, 2, 1), synth.normal(seed, 7, (B, D1, N)), f2))
    xyz1, xyz2, f1, f2 = (t.clone() for t in sets[0])

    def run():
        return fused(xyz1, xyz2, f1, f2)

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = run()
    for s in (sets[1], sets[0]):
        for dst, src in zip((xyz1, xyz2, f1, f2), s):
            dst.copy_(src)
        res.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = res.clone()
        eager = run()
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32)) and not torch.isnan(replayed).any()
        with torch.no_grad():
            compare_case({"out:new_points": replayed.cpu().numpy()}, {"out:new_points": mod(xyz1, xyz2, f1, f2).cpu().numpy()}, 1e-3,
                         "captured against the module")
