"""GPU tests (-m gpu) of the per-point attributes through the device data path: DevicePool(attr=...), resample_fps
(svnet_pool_gather_attr_f32, svnet_amd/csrc/fps.hip) and BatchLoader.points (the attribute instantiation of the batch kernel,
svnet_amd/csrc/batch.hip) against the numpy restatement tests/loader_attr_ref.py on top of tests/loader_ref.py.

`.points` is compared as BIT PATTERNS with the restatement evaluated in numpy float32 with the device's own `params` (every element,
no tolerance), and with the all-float64 restatement within 3 * ROT_BOUND + FP32_BOUND: three terms of (rotation-entry error, bounded
by ROT_BOUND as in tests/test_hip_loader.py) x (a component of magnitude <= 1), plus the fp32 bound derived in loader_attr_ref.py."""
import numpy as np
import pytest
import torch

from tests import loader_attr_ref as RA
from tests import loader_ref as R
from tests.common import compare_case

pytestmark = pytest.mark.gpu

SEED, NUM_CAT, B, M = 77, 16, 3, 7
AUGS = {"none": (False, "none"), "scale_shift": (True, "none"), "z": (False, "z"), "so3": (False, "so3"), "scale_shift_so3": (True, "so3")}
ROT_BOUND = 2e-6                                      # |rotation entry - float64 restatement|: tests/test_hip_loader.py
ATTRS = [(1, 0), (3, 1), (4, 1), (6, 2), (9, 1), (32, 0)]             # (A, attr_vectors)
PLANTED = 8                                           # points 0 .. 7 of every cloud carry the planted values

_POOLS, _ATTRS = {}, {}


def _arrays(P, M=M):
    if (P, M) not in _POOLS:
        rng = np.random.default_rng(2000 + P)
        _POOLS[P, M] = (rng.standard_normal((M, P, 3)).astype(np.float32), rng.integers(0, NUM_CAT, M), rng.integers(0, 50, (M, P)))
    return _POOLS[P, M]


def _attr(P, A, k, M=M):
    """[M,P,A]: k unit normals, then scalars; in every cloud the even points below PLANTED have a -0 in the first scalar channel (if
    there is one) and the odd ones a zero first vector (if there is one)."""
    if (P, A, k, M) not in _ATTRS:
        rng = np.random.default_rng(3000 + 100 * A + k + P)
        a = rng.standard_normal((M, P, A))
        for j in range(k):
            a[:, :, 3 * j:3 * j + 3] /= np.sqrt((a[:, :, 3 * j:3 * j + 3] ** 2).sum(-1, keepdims=True))
        a = a.astype(np.float32)
        if A > 3 * k:
            a[:, 0:PLANTED:2, 3 * k] = -0.0
        if k:
            a[:, 1:PLANTED:2, 0:3] = 0.0
        _ATTRS[P, A, k, M] = a
    return _ATTRS[P, A, k, M]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_points(loader, ref, attr, k, scale_shift, rotate, tag):
    """loader.points after a load against the restatement; returns the largest distance from the float64 restatement."""
    torch.cuda.synchronize()
    params = loader.params.cpu().numpy()
    got = loader.points.cpu().numpy()
    want = RA.points_fp32(attr, ref, params, k, scale_shift, rotate)
    same = _bits(got) == _bits(want)
    assert same.all(), "%s: %d of %d attribute values differ, first at %r" % (tag, (~same).sum(), same.size, np.argwhere(~same)[0])
    p64 = RA.points_f64(attr, ref, k, scale_shift)
    err = float(abs(got[:, :3 * k] - p64[:, :3 * k]).max()) if k else 0.0
    print("%s: direction channels against float64 %.3e (bound %.3e)" % (tag, err, 3 * ROT_BOUND + RA.FP32_BOUND))
    assert err <= 3 * ROT_BOUND + RA.FP32_BOUND, (tag, err)
    assert np.array_equal(got[:, 3 * k:], p64[:, 3 * k:].astype(np.float32))
    return err


def _untouched(loader):
    return [t.clone() for t in (loader.x, loader.y, loader.seg, loader.onehot, loader.params) if t is not None]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s,
                                                t.view(torch.int32) if t.dtype == torch.float32 else t) for s, t in zip(a, b))


@pytest.mark.parametrize("PN", [(64, 64), (96, 40), (2048, 1024)], ids=lambda v: "P%d_N%d" % v)
@pytest.mark.parametrize("aug", list(AUGS))
@pytest.mark.parametrize("select", R.SELECT)
def test_points_equal_the_restatement_and_the_other_buffers_are_untouched(select, aug, PN, hip_device):
    from svnet_amd.data import BatchLoader, DevicePool, epoch_order
    P, N = PN
    scale_shift, rotate = AUGS[aug]
    data, label, seg = _arrays(P)
    epoch = 5
    order = epoch_order(SEED, epoch, M)
    kw = dict(select=select, scale_shift=scale_shift, rotate=rotate, seed=SEED, num_cat=NUM_CAT)
    plain = BatchLoader(DevicePool(data, label, seg, device=hip_device), B, N, **kw)
    assert plain.points is None and plain.pool.A == 0 and plain.pool.attr is None
    plain.set_epoch(epoch)
    refs, base = [], []
    for step in (0, 1):
        assert plain.load(step) == B
        base.append(_untouched(plain))
        refs.append(R.batch(data, label, seg, seed=SEED, epoch=epoch, first=step * B, count=B, B=B, N=N, select=select,
                            scale_shift=scale_shift, rotate=rotate, order=order, num_cat=NUM_CAT))
    for A, k in ATTRS:
        attr = _attr(P, A, k)
        pool = DevicePool(data, label, seg, attr=attr, attr_vectors=k, device=hip_device)
        assert pool.A == A and pool.attr_vectors == k and tuple(pool.attr.shape) == (M, P, A)
        loader = BatchLoader(pool, B, N, **kw)
        assert tuple(loader.points.shape) == (B, A, N) and loader.points.dtype == torch.float32
        loader.set_epoch(epoch)
        loader.points.fill_(float("nan"))
        seen_negzero = seen_zero = False
        for step in (0, 1):
            assert loader.load(step) == B
            tag = (select, aug, PN, A, k, step)
            _check_points(loader, refs[step], attr, k, scale_shift, rotate, tag)
            assert _equal(_untouched(loader), base[step]), tag          # x, y, seg, onehot, params: what a pool without attributes gives
            got = loader.points.cpu().numpy()
            if A > 3 * k:
                seen_negzero |= bool((_bits(got[:, 3 * k]) == 0x80000000).any())
            if k:
                seen_zero |= bool((got[:, 0:3] == 0).all(1).any())
        assert seen_negzero == (A > 3 * k) and seen_zero == (k > 0), (select, aug, PN, A, k)     # the planted values were in the batches


def test_a_sample_does_not_depend_on_the_batching_and_a_short_batch_repeats_slot_zero(hip_device):
    from svnet_amd.data import BatchLoader, DevicePool
    P, N, A, k = 96, 40, 6, 2
    data, label, seg = _arrays(P)
    attr = _attr(P, A, k)
    pool = DevicePool(data, label, seg, attr=attr, attr_vectors=k, device=hip_device)
    for select in R.SELECT:
        kw = dict(select=select, scale_shift=True, rotate="so3", seed=SEED)
        three, one = BatchLoader(pool, B, N, **kw), BatchLoader(pool, 1, N, **kw)
        for ld in (three, one):
            ld.set_epoch(2)
        for step in range(len(three)):
            three.load(step)
            whole = three.points.clone()
            for b in range(B):
                one.load(step * B + b)
                assert torch.equal(one.points[0].view(torch.int32), whole[b].view(torch.int32)), (select, step, b)
        short = BatchLoader(pool, 4, N, drop_last=False, **kw)
        assert len(short) == 2
        short.points.fill_(float("nan"))
        assert short.load(1) == 3
        torch.cuda.synchronize()
        assert torch.equal(short.points[3].view(torch.int32), short.points[0].view(torch.int32))
        assert bool(torch.isfinite(short.points).all())
        ref = R.batch(data, label, seg, seed=SEED, epoch=0, first=4, count=3, B=4, N=N, select=select, scale_shift=True, rotate="so3",
                      order=R.epoch_order(SEED, 0, M))
        _check_points(short, ref, attr, k, True, "so3", (select, "short"))


def test_a_poisoned_order_entry_gives_nan_points(hip_device):
    from svnet_amd.data import BatchLoader, DevicePool
    data, label, seg = _arrays(64)
    pool = DevicePool(data, label, attr=_attr(64, 4, 1), attr_vectors=1, device=hip_device)
    loader = BatchLoader(pool, B, 64, select="first_shuffled", scale_shift=True, rotate="z", shuffle=False, seed=SEED)
    loader.order[1] = M                                                  # outside the pool: nothing is read
    loader.load(0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loader.points[1]).all()) and bool(torch.isnan(loader.x[1]).all())
    assert bool(torch.isfinite(loader.points[0]).all()) and bool(torch.isfinite(loader.points[2]).all())


def test_resample_fps_carries_the_attributes(hip_device):
    from svnet_amd.data import BatchLoader, DevicePool
    Mr, P, A, k, N = 3, 300, 6, 1, 64
    rng = np.random.default_rng(41)
    data = rng.standard_normal((Mr, P, 3)).astype(np.float32)
    label, seg = rng.integers(0, NUM_CAT, Mr), rng.integers(0, 50, (Mr, P))
    attr = _attr(P, A, k, M=Mr)
    big = DevicePool(data, label, seg, attr=attr, attr_vectors=k, device=hip_device)
    bare = DevicePool(data, label, seg, device=hip_device)
    for normalize in (False, True):
        new, ref = big.resample_fps(N, seed=3, normalize=normalize), bare.resample_fps(N, seed=3, normalize=normalize)
        torch.cuda.synchronize()
        assert new.A == A and new.attr_vectors == k and new.P == N and ref.A == 0 and ref.attr is None and ref.attr_vectors == 0
        idx = new.fps_index.cpu().numpy()
        assert np.array_equal(idx, ref.fps_index.cpu().numpy()) and torch.equal(new.seg, ref.seg)
        assert torch.equal(new.data.view(torch.int32), ref.data.view(torch.int32))
        want = np.stack([attr[m, idx[m]] for m in range(Mr)])
        assert tuple(new.attr.shape) == (Mr, N, A) and np.array_equal(_bits(new.attr.cpu().numpy()), _bits(want))
    # an index outside the cloud reads nothing: a NaN row
    from svnet_amd import _lib, _ops
    bad = new.fps_index.clone()
    bad[1, 5], bad[2, 0] = P, -1
    out = torch.zeros(Mr, N, A, device=hip_device)
    _lib.call("svnet_pool_gather_attr_f32", _ops._p(big.attr), _ops._p(bad), Mr, P, N, A, _ops._p(out), _ops._stream())
    torch.cuda.synchronize()
    nan = torch.isnan(out).all(-1).cpu().numpy()
    assert nan[1, 5] and nan[2, 0] and nan.sum() == 2 and not torch.isnan(out).any(-1).cpu().numpy()[~nan].any()
    # a loader on the result works
    loader = BatchLoader(new, Mr, 48, select="subset", scale_shift=True, rotate="so3", seed=SEED)
    loader.load(0)
    hd, ha = new.data.cpu().numpy(), new.attr.cpu().numpy()
    r = R.batch(hd, label, seed=SEED, epoch=0, first=0, count=Mr, B=Mr, N=48, select="subset", scale_shift=True, rotate="so3",
                order=R.epoch_order(SEED, 0, Mr))
    _check_points(loader, r, ha, k, True, "so3", "resampled")
    assert np.array_equal(_bits(loader.x.cpu().numpy()), _bits(R.x_fp32(hd, r, loader.params.cpu().numpy(), True, "so3")))


def test_loads_in_front_of_graph_replays_equal_eager_loads(hip_device):
    """A captured consumer of loader.points (its sum into a fixed scalar) replayed behind three loads: the buffers are the eager
    loads' bit for bit, and the replay sees three different batches."""
    from svnet_amd.data import BatchLoader, DevicePool
    data, label, seg = DevicePool.synthetic_arrays(3, 12, 256, 40)
    attr = _attr(256, 6, 2, M=12)
    pool = DevicePool(data, label, attr=attr, attr_vectors=2, device=hip_device)
    loader = BatchLoader(pool, 4, 128, select="first_shuffled", scale_shift=True, rotate="so3", seed=SEED)
    total = torch.zeros((), dtype=torch.float32, device=hip_device)
    eager = []
    for i in range(3):
        loader.load(i)
        total.copy_(loader.points.sum())
        eager.append((loader.points.clone(), loader.x.clone(), float(total)))
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        total.copy_(loader.points.sum())
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total.copy_(loader.points.sum())
    sums = []
    for i in range(3):
        loader.load(i)
        graph.replay()
        sums.append(float(total))
        assert torch.equal(loader.points.view(torch.int32), eager[i][0].view(torch.int32)), i
        assert torch.equal(loader.x.view(torch.int32), eager[i][1].view(torch.int32)), i
        assert sums[i] == eager[i][2], (i, sums[i], eager[i][2])
    assert all(np.isfinite(sums)) and len(set(sums)) == 3, sums


class _TwoLevels(torch.nn.Module):
    def __init__(self, num_class):
        super().__init__()
        from svnet_amd.models.utils.pointnet_util import PointNetSetAbstraction
        self.sa1 = PointNetSetAbstraction(16, 0.8, 8, 3 + 3, [16, 16], False)
        self.sa2 = PointNetSetAbstraction(None, None, None, 16 + 3, [32], True)
        self.fc = torch.nn.Linear(32, num_class)

    def forward(self, xyz, points):
        xyz1, feat1 = self.sa1(xyz, points)
        _, feat2 = self.sa2(xyz1, feat1)
        return self.fc(feat2.reshape(feat2.shape[0], 32))


def test_two_set_abstraction_levels_train_and_infer_on_loader_points(hip_device):
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.sa_fused import FusedSetAbstraction
    Me, P, N, Be = 8, 128, 64, 4
    data, label, _ = _arrays(P, Me)
    attr = _attr(P, 3, 1, M=Me)
    pool = DevicePool(data, label, attr=attr, attr_vectors=1, device=hip_device)
    loader = BatchLoader(pool, Be, N, select="first_shuffled", scale_shift=True, rotate="so3", seed=SEED)
    torch.manual_seed(0)
    model = _TwoLevels(NUM_CAT).to(hip_device).train()
    loader.load(1)

    def step(x, pts):
        model.zero_grad(set_to_none=True)
        logits = model(x, pts)
        loss = torch.nn.functional.cross_entropy(logits, loader.y)
        loss.backward()
        return logits.detach().clone(), loss.detach().clone()
    state = {n: t.clone() for n, t in model.state_dict().items()}
    logits, loss = step(loader.x, loader.points)
    grads = [p.grad for p in model.parameters()]
    assert bool(torch.isfinite(loss)) and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(p.grad.abs().max()) > 0 for p in model.sa1.parameters())
    model.load_state_dict(state)                                          # (the BatchNorm running statistics moved)
    logits2, loss2 = step(loader.x, loader.points)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    # fed from host copies of the restatement's tensors: the same logits
    params = loader.params.cpu().numpy()
    ref = R.batch(data, label, seed=SEED, epoch=0, first=Be, count=Be, B=Be, N=N, select="first_shuffled", scale_shift=True, rotate="so3",
                  order=R.epoch_order(SEED, 0, Me))
    hx = torch.from_numpy(R.x_fp32(data, ref, params, True, "so3")).to(hip_device)
    hp = torch.from_numpy(RA.points_fp32(attr, ref, params, 1, True, "so3")).to(hip_device)
    assert np.array_equal(loader.y.cpu().numpy(), ref["y"])
    model.load_state_dict(state)
    logits3, _ = step(hx, hp)
    assert torch.equal(logits.view(torch.int32), logits3.view(torch.int32))
    # inference: the fused first level takes loader.points
    model.eval()
    fused = FusedSetAbstraction(model.sa1)
    with torch.no_grad():
        mod_xyz, mod_points = model.sa1(loader.x, loader.points)
    new_xyz, new_points = fused(loader.x, loader.points)
    assert torch.equal(new_xyz.view(torch.int32), mod_xyz.view(torch.int32))
    compare_case({"out:new_points": new_points.cpu().numpy()}, {"out:new_points": mod_points.cpu().numpy()}, 1e-3, "fused first level")
