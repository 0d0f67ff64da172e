"""GPU tests (-m gpu) of the device-resident loader: svnet_batch_assemble_f32 (svnet_amd/csrc/batch.hip) through
svnet_amd.data.BatchLoader against the numpy restatement tests/loader_ref.py, and train_epoch / eval_epoch on top of it."""
import argparse
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import loader_ref as R

pytestmark = pytest.mark.gpu

SEED, NUM_CAT = 77, 16
AUGS = {"none": (False, "none"), "scale_shift": (True, "none"), "z": (False, "z"), "so3": (False, "so3"), "scale_shift_so3": (True, "so3")}
# |rotation entry - float64 restatement|: entries <= 1, products of two fp32 sqrt / sinpi / cospi results of a few ulp each, combined
# in a handful of fp32 operations: ~1e-6 worst case; the bound leaves a decade (largest value seen on MI355X: DESIGN.md)
ROT_BOUND = 2e-6

_POOLS = {}


def _arrays(P, M=7):
    if (P, M) not in _POOLS:
        rng = np.random.default_rng(1000 + P)
        data = rng.standard_normal((M, P, 3)).astype(np.float32)
        data[0, 0] = [-0.0, 0.0, -1.5]                                           # (signed zeros must survive "no augmentation")
        _POOLS[P, M] = (data, rng.integers(0, NUM_CAT, M), rng.integers(0, 50, (M, P)))
    return _POOLS[P, M]


def _pool(dev, P, with_seg, M=7):
    from svnet_amd.data import DevicePool
    data, label, seg = _arrays(P, M)
    return DevicePool(data, label, seg if with_seg else None, device=dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(loader, ref, data, scale_shift, rotate, tag):
    """Every buffer of `loader` after a load against the restatement `ref`; returns the largest rotation-entry error."""
    torch.cuda.synchronize()
    params = loader.params.cpu().numpy()
    x = loader.x.cpu().numpy()
    assert np.array_equal(loader.y.cpu().numpy(), ref["y"]), tag
    if loader.seg is not None:
        assert np.array_equal(loader.seg.cpu().numpy(), ref["seg"]), tag
    if loader.onehot is not None:
        assert np.array_equal(_bits(loader.onehot.cpu().numpy()), _bits(ref["onehot"])), tag
    assert np.array_equal(_bits(params[:, 0:3]), _bits(ref["scale"])), tag
    assert np.array_equal(_bits(params[:, 3:6]), _bits(ref["shift"])), tag
    assert (params[:, 15] == 0).all()
    rot_err = float(abs(params[:, 6:15].astype(np.float64) - ref["R"].reshape(-1, 9)).max())
    assert rot_err <= ROT_BOUND, (tag, rot_err)
    if rotate == "none":
        assert rot_err == 0.0
    # x with the device's own params, in fp32, same operation order: bit-identical - which also pins the point order
    want = R.x_fp32(data, ref, params, scale_shift, rotate)
    same = _bits(x) == _bits(want)
    assert same.all(), "%s: %d of %d coordinates differ, first at %r" % (tag, (~same).sum(), same.size, np.argwhere(~same)[0])
    # and close to the all-float64 restatement: three terms of (rotation-entry error x coordinate), plus fp32 rounding of the rest
    assert abs(x - ref["x"]).max() <= 3 * ROT_BOUND * abs(ref["x"]).max() + 1e-5, tag
    return rot_err


@pytest.mark.parametrize("PN", [(64, 64), (2048, 1024), (2048, 2048), (4096, 1024)], ids=lambda v: "P%d_N%d" % v)
@pytest.mark.parametrize("aug", list(AUGS))
@pytest.mark.parametrize("select", R.SELECT)
def test_batch_equals_the_restatement(select, aug, PN, hip_device):
    from svnet_amd.data import BatchLoader, epoch_order
    P, N = PN
    scale_shift, rotate = AUGS[aug]
    data, label, seg = _arrays(P)
    M, B, epoch = data.shape[0], 3, 5
    order = epoch_order(SEED, epoch, M)
    assert np.array_equal(order, R.epoch_order(SEED, epoch, M))
    worst = 0.0
    for with_extras in (False, True):
        pool = _pool(hip_device, P, with_extras)
        loader = BatchLoader(pool, B, N, select=select, scale_shift=scale_shift, rotate=rotate, seed=SEED,
                             num_cat=NUM_CAT if with_extras else None)
        assert (loader.seg is not None) == with_extras and (loader.onehot is not None) == with_extras and len(loader) == M // B
        loader.set_epoch(epoch)
        for step in (0, 1):
            assert loader.load(step) == B
            ref = R.batch(data, label, seg if with_extras else None, seed=SEED, epoch=epoch, first=step * B, count=B, B=B, N=N,
                          select=select, scale_shift=scale_shift, rotate=rotate, order=order, num_cat=NUM_CAT if with_extras else None)
            worst = max(worst, _check(loader, ref, data, scale_shift, rotate, (select, aug, PN, with_extras, step)))
    print("largest rotation-entry error vs float64 (%s, %s, P %d, N %d): %.3e" % (select, aug, P, N, worst))


@pytest.mark.parametrize("rotate", ["z", "so3"])
def test_rotation_entries_over_many_clouds(rotate, hip_device):
    """The rotation entries of 4096 clouds (two epochs of 2048) against the float64 restatement, and proper rotations in fp32."""
    from svnet_amd.data import BatchLoader, DevicePool
    M, B = 2048, 256
    rng = np.random.default_rng(8)
    pool = DevicePool(rng.standard_normal((M, 4, 3)).astype(np.float32), rng.integers(0, 40, M), device=hip_device)
    loader = BatchLoader(pool, B, 4, select="first_ordered", scale_shift=False, rotate=rotate, seed=SEED)
    worst = 0.0
    for epoch in (0, 9):
        loader.set_epoch(epoch)
        for step in range(len(loader)):
            loader.load(step)
            got = loader.params.cpu().numpy()[:, 6:15].astype(np.float64).reshape(B, 3, 3)
            want = np.stack([R.rotation_of(R.cloud_key(SEED, epoch, step * B + b), rotate) for b in range(B)])
            worst = max(worst, float(abs(got - want).max()))
            assert abs(got @ got.transpose(0, 2, 1) - np.eye(3)).max() < 4 * ROT_BOUND and abs(np.linalg.det(got) - 1).max() < 4 * ROT_BOUND
    print("largest rotation-entry error vs float64 over 4096 clouds (%s): %.3e" % (rotate, worst))
    assert worst <= ROT_BOUND, worst


def _snapshot(loader):
    return [t.clone() for t in (loader.x, loader.y, loader.seg, loader.onehot, loader.params) if t is not None]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s,
                                                t.view(torch.int32) if t.dtype == torch.float32 else t) for s, t in zip(a, b))


@pytest.mark.parametrize("select", R.SELECT)
def test_a_sample_does_not_depend_on_the_batching(select, hip_device):
    """The same 8 positions of the epoch order as one batch of 8 (world 1) and as two ranks' batches of 4 (both on this GPU)."""
    from svnet_amd.data import BatchLoader
    pool = _pool(hip_device, 2048, True, M=20)
    kw = dict(select=select, scale_shift=True, rotate="so3", seed=SEED, num_cat=NUM_CAT)
    one = BatchLoader(pool, 8, 1024, **kw)
    ranks = [BatchLoader(pool, 4, 1024, rank=r, world=2, **kw) for r in range(2)]
    for ld in [one] + ranks:
        ld.set_epoch(2)
    for step in range(len(one)):
        assert one.load(step) == 8 and all(ld.load(step) == 4 for ld in ranks)
        whole = _snapshot(one)
        parts = [torch.cat(pair, dim=0) for pair in zip(_snapshot(ranks[0]), _snapshot(ranks[1]))]
        assert _equal(whole, parts), step
    assert len(one) == 2 and len(ranks[0]) == 2
    one.load(0)
    a = _snapshot(one)
    one.load(0)
    assert _equal(a, _snapshot(one))                          # load(step) twice: identical buffers
    one.load(1)
    assert not torch.equal(a[0], one.x)
    one.set_epoch(3)
    one.load(0)
    assert not torch.equal(a[0], one.x)                       # another epoch: another order and another augmentation


def test_short_final_batch_repeats_slot_zero(hip_device):
    from svnet_amd.data import BatchLoader
    data, label, seg = _arrays(2048, 7)
    pool = _pool(hip_device, 2048, True)
    for select, shuffle in (("first_ordered", False), ("subset", True)):
        loader = BatchLoader(pool, 4, 1024, select=select, scale_shift=shuffle, rotate="z" if shuffle else "none", shuffle=shuffle,
                             drop_last=False, seed=SEED, num_cat=NUM_CAT)
        assert len(loader) == 2
        for t in (loader.x, loader.params, loader.onehot):
            t.fill_(float("nan"))                              # whatever the launch does not write stays visible
        assert loader.load(0) == 4 and loader.load(1) == 3
        torch.cuda.synchronize()
        for t in _snapshot(loader):
            assert torch.equal(t[3], t[0])
            assert bool(torch.isfinite(t.double()).all())
        order = R.epoch_order(SEED, 0, 7) if shuffle else np.arange(7)
        ref = R.batch(data, label, seg, seed=SEED, epoch=0, first=4, count=3, B=4, N=1024, select=select, scale_shift=shuffle,
                      rotate="z" if shuffle else "none", order=order, num_cat=NUM_CAT)
        _check(loader, ref, data, shuffle, "z" if shuffle else "none", (select, "short"))
        with pytest.raises(IndexError):
            loader.load(2)


def _model(dev, k=8):
    import svnet_amd.models as M
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return M.SV_DGCNN_CLS(argparse.Namespace(k=k, binary=True), 40).to(dev).train()


def test_launches_between_graph_replays_equal_eager_launches(hip_device):
    """Steps 0..2 launched eagerly, then the same steps launched in front of the replays of a captured TrainStep that reads the
    loader's buffers: the same batches bit for bit, and the replay sees them (three different losses)."""
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.train import TrainStep
    pool = DevicePool.synthetic(3, 12, 256, 40, device=hip_device)
    loader = BatchLoader(pool, 4, 128, select="first_shuffled", scale_shift=True, rotate="so3", seed=SEED)
    eager = []
    for i in range(3):
        loader.load(i)
        eager.append(_snapshot(loader))
    step = TrainStep(_model(hip_device), (loader.x,), loader.y).capture()
    losses = []
    for i in range(3):
        loader.load(i)
        losses.append(float(step.run(all_reduce=False)))
        assert _equal(eager[i], _snapshot(loader)), i
    assert all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    loader.load(0)
    assert float(step.run(all_reduce=False)) == losses[0]      # (the forward is reproducible: the same batch, the same loss)


def test_train_epoch_and_eval_epoch(hip_device):
    from svnet_amd.data import BatchLoader, DevicePool
    from svnet_amd.train import FlatAdam, FlatParams, ForwardStep, TrainStep, eval_epoch, train_epoch
    pool = DevicePool.synthetic(4, 12, 256, 40, device=hip_device)
    kw = dict(select="first_shuffled", scale_shift=True, rotate="z", seed=SEED)
    loader, twin = BatchLoader(pool, 4, 128, **kw), BatchLoader(pool, 4, 128, **kw)
    assert len(loader) == 3
    model = _model(hip_device)
    fp = FlatParams(model)
    step = TrainStep(model, (loader.x,), loader.y).capture()
    opt = FlatAdam(fp, step.bucket, lr=1e-3)
    seen, losses = [], []

    class Spy:
        def run(self):
            seen.append((loader.x.clone(), loader.y.clone()))
            loss = step.run()
            losses.append(loss.clone())
            return loss
    before = fp.flat.clone()
    for ld in (loader, twin):
        ld.set_epoch(1)
    mean = train_epoch(Spy(), loader, opt)
    torch.cuda.synchronize()
    assert len(seen) == 3 and opt.steps == 3
    for i, (x, y) in enumerate(seen):
        twin.load(i)
        assert torch.equal(x.view(torch.int32), twin.x.view(torch.int32)) and torch.equal(y, twin.y), i
    vals = [float(v) for v in losses]
    assert all(np.isfinite(vals)) and abs(mean - sum(vals) / 3) < 1e-5 * max(1.0, abs(mean)), (mean, vals)
    assert bool(torch.isfinite(fp.flat).all()) and not torch.equal(before, fp.flat)

    pool10 = DevicePool.synthetic(5, 10, 256, 40, device=hip_device)
    ev = BatchLoader(pool10, 4, 128, select="first_ordered", scale_shift=False, rotate="none", shuffle=False, drop_last=False, seed=SEED)
    assert len(ev) == 3
    fwd = ForwardStep(model, (ev.x,))
    logits, pred = eval_epoch(fwd, ev)
    assert tuple(logits.shape) == (10, 40) and tuple(pred.shape) == (10,) and bool(torch.isfinite(logits).all())
    # the rows are the model's eval-mode logits of the pool's clouds in pool order (eval-mode BatchNorm: no batch coupling)
    ev.load(2)
    again = fwd.run()
    assert torch.equal(again[:2], logits[8:10])
    x_direct = pool10.data[8:10, :128].permute(0, 2, 1).contiguous()
    assert torch.equal(ev.x[:2], x_direct)
