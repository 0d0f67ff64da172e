"""GPU tests (-m gpu) of the multi-scale grouping: svnet_ball_query_msg_f32, svnet_group_points_msg_f32 and
svnet_group_points_msg_bwd_f32 (svnet_amd/csrc/group.hip) through svnet_amd.group, and PointNetSetAbstractionMsg of
svnet_amd/models/utils/pointnet_msg.py, against the numpy restatement tests/msg_ref.py, the single-scale calls on the device and the
reference's recorded results (tests/golden/msg.npz).  The contract is single-rounded fp32 with a fixed sum order, so indices and counts
are compared as integers and everything else as BIT PATTERNS; the two tolerances there are, are derived where they are used.  Every
case runs at B = 2; every reference is computed once per process and shared."""
import os

import numpy as np
import pytest
import torch

from svnet_amd import synth
from tests import group_ref as G
from tests import msg_ref as M
from tests.common import compare_case

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msg.npz"))
F32 = np.float32
B = 2
_REF = {}


def _tile():
    try:
        from svnet_amd import group as Gr
        return Gr.tile()
    except Exception:                 # the library or the module is missing: the tests still fail, at the import in the test
        return 2048


T = _tile()
# (N, S, radii, nsamples, D): every N in {1, 2, 63, 64, 65, 129, tile - 1, tile, tile + 1, 2 tile + 5}, every S in {1, 3, 5, 130}
# (partial workgroups of four waves x eight centres), every R in {1, 2, 3, 4} and every D in {0, 1, 5, 61, 64} (rows of 3, 4, 8, 64
# and 67 columns: the float4 and the dword path) at least once.  Radii are un-sorted and repeat (0.8, 0.2 and 0.5 with two nsample).
# Where N allows it a list mixes a scale that fills within the first 64 candidates (radius 3 or 4 takes every point), one that fills
# late - in a later LDS tile where N >= 2 tile - and one that never fills (radius 0.05); centre 1 is planted far from the cloud where
# S >= 3: the empty group, in every scale.
CASES = [(1, 1, (0.4,), (1,), 0),
         (2, 3, (0.8, 0.8), (2, 1), 1),
         (63, 5, (0.9, 0.3, 1.5), (63, 8, 16), 5),
         (64, 130, (1.5, 0.2, 0.6, 0.2), (64, 4, 16, 9), 61),
         (65, 3, (0.9, 3.0), (65, 5), 64),
         (129, 5, (0.5, 0.05, 4.0), (16, 8, 40), 0),
         (T - 1, 130, (4.0, 0.5, 0.05, 0.5), (4, 100, 8, 37), 1),
         (T, 5, (0.4, 4.0), (63, 2), 5),
         (T + 1, 3, (0.4, 0.05, 4.0), (65, 8, 64), 61),
         (2 * T + 5, 130, (0.05, 4.0, 0.5, 0.5), (8, 4, 200, 64), 64),
         (2 * T + 5, 5, (0.3, 0.05, 3.0), (150, 2, 6), 5),
         (129, 1, (1.0,), (128,), 0),
         # one scale WITH attributes: the one-scale, attributes-first forms of the grouping and of its gradient
         (65, 33, (0.9,), (5,), 1),                # float4 rows, one centre past a 32-centre workgroup
         (T + 1, 3, (0.4,), (65,), 5),             # the second LDS tile, a list longer than a 64-candidate step
         (64, 7, (1.5,), (64,), 61)]               # rows of 64 columns
GRAD_CASES = [c for c in CASES if c[4] > 0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same_bits(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got, want) if got.dtype != F32 else (_bits(got), _bits(want))
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %r: got %r, want %r" % (
        tag, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _once(key, make):
    if key not in _REF:
        res = make()
        for a in res:
            for v in (a if isinstance(a, list) else [a]):
                if v is not None:
                    v.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def _dev(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev) for a in arrays)      # a copy: the references are read-only


def _inputs(kind, N, S, D):
    def make():
        x, c, pts = (G.lattice_case if kind == "lattice" else G.gauss_case)(7000 + N + S, B, N, S, D)
        if S >= 3:
            c[:, 1] = 9.0                                            # planted: no point within any radius used here
        return x, np.ascontiguousarray(c), pts
    return _once(("in", kind, N, S, D), make)


def _forward_ref(kind, N, S, radii, nsamples, D):
    def make():
        x, c, pts = _inputs(kind, N, S, D)
        idx_cat, count = M.query_ball_msg_batch(x, c, [G.r2_of(r) for r in radii], nsamples)
        return idx_cat, count, M.group_msg_batch(x, c, idx_cat, nsamples, pts)
    return _once(("fwd", kind, N, S, radii, nsamples, D), make)


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("N,S,radii,nsamples,D", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_query_and_grouping_equal_the_restatement_and_the_single_scale_calls(N, S, radii, nsamples, D, kind, hip_device):
    from svnet_amd import group as Gr
    dev, R, Ktot = hip_device, len(radii), sum(nsamples)
    x, c, pts = _inputs(kind, N, S, D)
    want_idx, want_count, want_out = _forward_ref(kind, N, S, radii, nsamples, D)
    tag = "%s N %d S %d radii %s nsample %s D %d" % (kind, N, S, radii, nsamples, D)
    tx, tc, tp = _dev(dev, x, c, pts)
    # 1. the restatement, as integers
    idx_cat, count = Gr.query_ball_point_msg(radii, nsamples, tx, tc, return_count=True)
    assert idx_cat.dtype == torch.int64 and tuple(idx_cat.shape) == (B, S, Ktot) and count.dtype == torch.int32 and tuple(count.shape) == (B, S, R)
    assert torch.equal(idx_cat, Gr.query_ball_point_msg(radii, nsamples, tx, tc))
    got_idx, got_count = idx_cat.cpu().numpy(), count.cpu().numpy()
    _same_bits(got_idx, want_idx, tag + " idx_cat")
    _same_bits(got_count, want_count, tag + " count")
    assert ((got_idx >= 0) & (got_idx < N)).all()
    if S >= 3:
        assert (got_count[:, 1] == 0).all() and (got_idx[:, 1] == 0).all()                       # the empty group, in every scale
    assert (got_count[:, 0] >= 1).all()                                                         # centre 0 is a point: it finds itself
    last = np.stack([v[..., -1] for v in M.split(want_idx, nsamples)], axis=-1)
    full = want_count == np.array(nsamples)
    if N >= 129 and R >= 3:
        assert (full & (last < 64)).any() and (~full).any(), tag                               # fills in the first step; never fills
    if N >= 2 * T and R >= 3:
        assert (full & (last >= T)).any(), tag                                                  # fills in a later tile
    # 2. every scale is the single-scale call on the device
    views = Gr.split_scales(idx_cat, nsamples)
    for i, (radius, k) in enumerate(zip(radii, nsamples)):
        one_idx, one_count = Gr.query_ball_point(radius, k, tx, tc, return_count=True)
        assert torch.equal(views[i], one_idx) and torch.equal(count[..., i], one_count), "%s scale %d" % (tag, i)
        for j in range(i):
            if radii[j] == radius:                                                              # a repeated radius: the shorter list is a prefix
                a, b = (views[i], views[j]) if k <= nsamples[j] else (views[j], views[i])
                assert torch.equal(a, b[..., :a.shape[2]]), "%s scales %d, %d" % (tag, j, i)
    # 3. the grouped tensors: the restatement's bits, and group_points with its columns rotated
    outs = Gr.group_points_msg(tx, tc, idx_cat, nsamples, tp)
    assert isinstance(outs, tuple) and len(outs) == R
    for i, k in enumerate(nsamples):
        assert outs[i].dtype == torch.float32 and tuple(outs[i].shape) == (B, S, k, D + 3) and outs[i].is_contiguous()
        _same_bits(outs[i].cpu().numpy(), want_out[i], "%s grouped %d" % (tag, i))
        one = Gr.group_points(tx, tc, views[i].contiguous(), tp)
        assert torch.equal(torch.cat([one[..., 3:], one[..., :3]], dim=-1).view(torch.int32), outs[i].view(torch.int32)), "%s scale %d" % (tag, i)
    far = idx_cat.clone()
    far[:, :, 0], far[:, :, -1] = -7, N + 3                                                      # clamped, never followed
    clamped = idx_cat.clone()
    clamped[:, :, 0], clamped[:, :, -1] = 0, N - 1
    for a, b in zip(Gr.group_points_msg(tx, tc, far, nsamples, tp), Gr.group_points_msg(tx, tc, clamped, nsamples, tp)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    per, union = M.scanned_fraction(want_idx, want_count, list(nsamples), N)
    print("%s: full groups per scale %s, scanned fraction per scale %s, union %.3f"
          % (tag, full.reshape(-1, R).sum(axis=0).tolist(), ["%.3f" % f for f in per], union))


def _autograd_gradient(tp, idx_cat, nsamples, grads):
    """The gradient of sum_i <points[idx_i], g_i[..., :D]> by torch's autograd through index_select."""
    (Bc, N, D), leaf = tp.shape, tp.clone().requires_grad_()
    flat = leaf.reshape(Bc * N, D)
    shift = (torch.arange(Bc, device=tp.device) * N).view(Bc, 1, 1)
    loss = 0
    for idx, g in zip(torch.split(idx_cat, list(nsamples), dim=2), grads):
        sel = flat.index_select(0, (idx.clamp(0, N - 1) + shift).reshape(-1)).view(Bc, idx.shape[1], idx.shape[2], D)
        loss = loss + (sel * g[..., :D]).sum()
    return torch.autograd.grad(loss, leaf)[0]


@pytest.mark.parametrize("kind", ["lattice", "gauss"])
@pytest.mark.parametrize("N,S,radii,nsamples,D", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_backward_equals_the_restatement_and_autograd(N, S, radii, nsamples, D, kind, hip_device):
    from svnet_amd import group as Gr
    dev = hip_device
    x, c, pts = _inputs(kind, N, S, D)
    idx_np = _forward_ref(kind, N, S, radii, nsamples, D)[0]
    seed = 7100 + N + S

    def make():
        gs = [synth.normal(seed, 10 + i, (B, S, k, D + 3)) for i, k in enumerate(nsamples)]
        want = M.group_msg_bwd_batch(gs, idx_np, nsamples, N)
        exact, bound = zip(*(M.group_msg_bwd_f64([g[b] for g in gs], idx_np[b], nsamples, N) for b in range(B)))
        return gs, want, np.stack(exact), np.stack(bound)
    gs, want, exact, bound = _once(("bwd", kind, N, S, radii, nsamples, D), make)
    tag = "%s N %d S %d nsample %s D %d" % (kind, N, S, nsamples, D)
    tx, tc, tp, ti = _dev(dev, x, c, pts, idx_np)
    tg = _dev(dev, *gs)
    # 4. the restatement's bits, into a NaN-filled buffer; a second run; through .backward()
    buf = torch.full((B, N, D), float("nan"), dtype=torch.float32, device=dev)
    got = Gr.group_points_msg_backward(tg, ti, nsamples, N, out=buf)
    assert got is buf
    _same_bits(got.cpu().numpy(), want, tag + " group_points_msg_backward")
    again = Gr.group_points_msg_backward(tg, ti, nsamples, N)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    plain = Gr.group_points_msg(tx, tc, ti, nsamples, tp)
    leaf = tp.clone().requires_grad_()
    outs = Gr.group_points_msg(tx, tc, ti, nsamples, leaf)
    assert all(o.requires_grad and torch.equal(o.detach().view(torch.int32), p.view(torch.int32)) for o, p in zip(outs, plain))
    torch.autograd.backward(outs, tg)
    _same_bits(leaf.grad.cpu().numpy(), want, tag + " .backward()")
    # torch's autograd through index_select adds in no fixed order: both results lie within the bound of tests/pointset_grad_ref.py,
    # L 2^-23 sum|t_i|, of the float64 sum, and - each being at most (L - 1) 2^-24 sum|t_i| off - of each other
    auto = _autograd_gradient(tp, ti, nsamples, tg).cpu().numpy()
    mine = got.cpu().numpy()
    err, off = np.abs(mine - exact), np.abs(mine.astype(np.float64) - auto)
    print("%s: |got - f64| at most %.3f of the bound, |got - autograd| %.3f" % (
        tag, float((err / np.maximum(bound, 1e-300)).max()), float((off / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all() and (off <= bound).all(), tag
    # integer upstream gradients in -4 .. 4: every sum is exact, whatever its order - autograd's bits
    ints = [(synth.integers(seed, 20 + i, (B, S, k, D + 3), 9) - 4).astype(F32) for i, k in enumerate(nsamples)]
    ti_g = _dev(dev, *ints)
    _same_bits(Gr.group_points_msg_backward(ti_g, ti, nsamples, N).cpu().numpy(), _autograd_gradient(tp, ti, nsamples, ti_g).cpu().numpy(),
               tag + " integer gradients against autograd")


# ---- the reference's recorded results
@pytest.mark.parametrize("name", list(M.GOLDEN_CASES))
def test_golden_indices_and_grouped_tensors_bit_for_bit(name, hip_device):
    from svnet_amd import group as Gr
    seed, Bc, N, S, radii, nsamples, D, _ = M.GOLDEN_CASES[name]
    x, c = GOLDEN[name + "_xyz"], GOLDEN[name + "_new_xyz"]
    pts = GOLDEN[name + "_points"] if D else None
    tx, tc, tp, start = _dev(hip_device, x, c, pts, GOLDEN[name + "_start"])
    idx_cat, count = Gr.query_ball_point_msg(radii, nsamples, tx, tc, return_count=True)
    outs = Gr.group_points_msg(tx, tc, idx_cat, nsamples, tp)
    new_xyz, sampled = Gr.sample_and_group_msg(S, radii, nsamples, tx, tp, start=start)
    _same_bits(new_xyz.cpu().numpy(), c, name + " new_xyz")
    assert (count >= 1).all()
    for i, view in enumerate(Gr.split_scales(idx_cat, nsamples)):
        _same_bits(view.cpu().numpy(), GOLDEN["%s_idx%d" % (name, i)].astype(np.int64), "%s idx %d" % (name, i))
        _same_bits(outs[i].cpu().numpy(), GOLDEN["%s_grouped%d" % (name, i)], "%s grouped %d" % (name, i))
        _same_bits(sampled[i].cpu().numpy(), GOLDEN["%s_grouped%d" % (name, i)], "%s sample_and_group_msg %d" % (name, i))


@pytest.mark.parametrize("mode", ["ev", "tr"])
@pytest.mark.parametrize("name", list(M.GOLDEN_CASES))
def test_module_equals_the_recorded_reference(name, mode, hip_device):
    """PointNetSetAbstractionMsg with the recorded state_dict (strict), eval and train mode: outputs, loss and gradients against the
    reference's within 1e-3 under tests.common.compare_case, the figure tests/golden/pointset_grad.npz is held to; the sampled
    centres bit for bit.  (Train mode holds no gradient of a convolution's bias: tests/golden/make_msg_golden.py says why.)"""
    from svnet_amd.models.utils import pointnet_msg as U
    dev = hip_device
    seed, Bc, N, S, radii, nsamples, D, mlp_list = M.GOLDEN_CASES[name]
    mod = U.PointNetSetAbstractionMsg(S, list(radii), list(nsamples), D, [list(m) for m in mlp_list])
    mod.load_state_dict({str(k): torch.from_numpy(GOLDEN["%s_sd:%s" % (name, k)]) for k in GOLDEN[name + "_keys"]}, strict=True)
    mod.to(dev).train(mode == "tr")
    xyz, lw, start = _dev(dev, GOLDEN[name + "_xyz"].transpose(0, 2, 1), GOLDEN[name + "_lw"], GOLDEN[name + "_start"])
    pts = _dev(dev, GOLDEN[name + "_points"].transpose(0, 2, 1))[0].requires_grad_() if D else None
    new_xyz, new_points = mod(xyz, pts, start=start)
    loss = (new_points * lw).sum()
    loss.backward()
    got = {"out:new_xyz": new_xyz.detach().cpu().numpy(), "out:new_points": new_points.detach().cpu().numpy(),
           "out:loss": np.array([float(loss.detach())])}
    if D:
        got["dx:points"] = pts.grad.cpu().numpy()
    for k, p in mod.named_parameters():
        got["d:" + k] = p.grad.cpu().numpy()
    prefix = "%s_%s_" % (name, mode)
    ref = {k[len(prefix):]: GOLDEN[k] for k in GOLDEN.files if k.startswith(prefix)}
    assert set(ref) <= set(got) and {k for k in got if k not in ref} == ({k for k in got if k.startswith("d:conv_blocks.") and k.endswith(".bias")}
                                                                         if mode == "tr" else set())
    assert np.array_equal(_bits(got["out:new_xyz"]), _bits(ref["out:new_xyz"]))
    worst = compare_case(got, ref, 1e-3, "%s %s" % (name, mode))
    print("%s %s: worst relative error %.3e at %s" % ((name, mode) + worst))


# ---- a captured graph
def test_sample_and_group_msg_in_a_captured_graph(hip_device):
    """sample_and_group_msg with a device start captured on a side stream after a warm-up; two replays with the inputs refilled in
    place between them each give the eager result bit for bit."""
    from svnet_amd import group as Gr
    dev = hip_device
    N, S, D, radii, nsamples = 300, 33, 5, (0.4, 0.1, 0.4), (16, 4, 7)
    sets = []
    for seed in (90, 91):
        x, _, pts = G.gauss_case(seed, B, N, 4, D)
        sets.append(_dev(dev, x, pts, np.array([seed % 7, 200 + seed % 5], dtype=np.int64)))
    x, pts, start = (t.clone() for t in sets[0])

    def run():
        new_xyz, grouped = Gr.sample_and_group_msg(S, radii, nsamples, x, pts, start=start)
        return (new_xyz,) + tuple(grouped)

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
        for dst, src in zip((x, pts, start), s):
            dst.copy_(src)
        for r in res:
            r.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = [r.clone() for r in res]
        eager = run()
        assert len(replayed) == 1 + len(nsamples)
        for a, b in zip(replayed, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.isnan(a).any()
