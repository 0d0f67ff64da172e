"""CPU tests of the device-resident loader's host side (svnet_amd/data.py, the batch entry points of libsvnet_hip.so) and of the
numpy restatement the GPU tests compare against (tests/loader_ref.py)."""
import ctypes

import numpy as np
import pytest

from tests import loader_ref as R


def test_batch_supported_answers_without_a_gpu():
    from svnet_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 2):
        assert L.svnet_batch_supported(2048, 1024, mode) == 1
        assert L.svnet_batch_supported(2048, 2048, mode) == 1
        assert L.svnet_batch_supported(1024, 2048, mode) == 0            # N > P
        assert L.svnet_batch_supported(0, 0, mode) == 0
    assert L.svnet_batch_supported(16384, 1024, 1) == 0                  # SUBSET sorts S = P = 16 384 keys: 128 KiB
    assert L.svnet_batch_supported(16384, 1024, 0) == 1                  # FIRST_SHUFFLED sorts S = N keys
    assert L.svnet_batch_supported(16384, 16384, 0) == 0
    assert L.svnet_batch_supported(16384, 16384, 2) == 1                 # FIRST_ORDERED sorts nothing
    assert L.svnet_batch_supported(8192, 8192, 1) == 1 and L.svnet_batch_supported(8193, 8193, 1) == 0       # 64 KiB of keys
    assert L.svnet_batch_supported(2048, 1024, 3) == 0 and L.svnet_batch_supported(2048, 1024, -1) == 0


def _desc(**over):
    """A descriptor whose pointers are non-null host addresses: only argument checks may look at it (nothing is launched)."""
    from svnet_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.BatchDesc()
    d._keep = buf
    d.data = d.label = d.seg = d.order = d.x = d.y = d.seg_out = d.onehot = d.params = p
    d.M, d.P, d.L, d.B, d.N, d.first, d.count, d.seed, d.epoch = 10, 2048, 10, 4, 1024, 0, 4, 1, 0
    d.select_mode, d.scale_shift, d.rotate, d.num_cat = 0, 1, 0, 16
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over, word", [
    (dict(data=None), b"null"), (dict(order=None), b"null"), (dict(x=None), b"null"), (dict(params=None), b"null"),
    (dict(seg=None), b"seg"),                          # seg_out without a pool seg
    (dict(N=4096), b"N 4096 > P 2048"),
    (dict(count=5), b"count"), (dict(count=0), b"count"),
    (dict(first=8), b"first"), (dict(first=-1), b"first"),
    (dict(select_mode=7), b"select_mode"), (dict(rotate=3), b"rotate"),
    (dict(num_cat=0), b"num_cat"),
    (dict(M=0), b"positive"),
])
def test_argument_errors_return_minus_one_with_a_message(over, word):
    from svnet_amd import _lib
    L = _lib.lib()
    assert L.svnet_batch_assemble_f32(ctypes.byref(_desc(**over)), None) == -1
    assert word in L.svnet_last_error(), L.svnet_last_error()
    assert L.svnet_batch_assemble_f32(None, None) == -1 and b"null" in L.svnet_last_error()


def test_unsupported_shape_is_refused_before_any_launch():
    from svnet_amd import _lib
    L = _lib.lib()
    assert L.svnet_batch_assemble_f32(ctypes.byref(_desc(P=16384, select_mode=1)), None) == -2
    assert b"64 KiB" in L.svnet_last_error()


def test_epoch_order_is_a_permutation_and_equals_the_restatement():
    from svnet_amd.data import epoch_order
    for M in (1, 2, 103, 9840):
        o = epoch_order(1234, 3, M)
        assert o.dtype == np.int64 and np.array_equal(np.sort(o), np.arange(M))
    for seed, epoch, M in ((1234, 3, 103), (0, 0, 64), (2 ** 63 - 1, 2 ** 40, 500)):
        assert np.array_equal(epoch_order(seed, epoch, M), R.epoch_order(seed, epoch, M))
    a = epoch_order(1234, 3, 1000)
    assert not np.array_equal(a, epoch_order(1234, 4, 1000)) and not np.array_equal(a, epoch_order(1235, 3, 1000))
    assert not np.array_equal(a, np.arange(1000))


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("drop_last", [True, False])
def test_rank_partition(world, drop_last):
    from svnet_amd.data import batch_span, steps_per_epoch
    M, B = 103, 4
    steps = steps_per_epoch(M, B, world, drop_last)
    taken, valid = [], 0
    for rank in range(world):
        for step in range(steps):
            first, count = batch_span(M, B, step, rank, world)
            assert 0 <= count <= B and (count == 0 or first + count <= M)
            taken += list(range(first, first + count))
            valid += count
    assert len(set(taken)) == len(taken)                                             # disjoint
    if drop_last:
        assert sorted(taken) == list(range(world * B * steps)) and world * B * steps <= M < world * B * (steps + 1)
    else:
        assert valid == M and sorted(taken) == list(range(M))


def test_loader_needs_a_hip_pool():
    from svnet_amd.data import DevicePool
    data, label, seg = DevicePool.synthetic_arrays(3, 5, 32, 40, 50)
    assert data.shape == (5, 32, 3) and data.dtype == np.float32 and label.shape == (5,) and seg.shape == (5, 32)
    with pytest.raises(RuntimeError):
        DevicePool(data, label, seg, device="cpu")
    with pytest.raises(TypeError):
        DevicePool(data.astype(np.float64), label, device="cpu")
    with pytest.raises(ValueError):
        DevicePool(data, label[:4], device="cpu")
    with pytest.raises(ValueError):
        DevicePool(data, label, seg[:, :8], device="cpu")


# ----------------------------------------------------------------------------- the restatement itself (tests/loader_ref.py)

def _pool(M=6, P=96, seed=5):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((M, P, 3)).astype(np.float32)
    assert len(np.unique(data.reshape(-1, 3), axis=0)) == M * P                      # distinct rows: a point identifies its source
    return data, rng.integers(0, 16, M), rng.integers(0, 50, (M, P))


@pytest.mark.parametrize("select", ["first_shuffled", "subset", "first_ordered"])
@pytest.mark.parametrize("rotate", ["none", "z", "so3"])
def test_restatement_rearranges_pool_points_with_bounded_augmentation(select, rotate):
    data, label, seg = _pool()
    M, P, N = data.shape[0], data.shape[1], 64
    order = R.epoch_order(9, 1, M)
    ref = R.batch(data, label, seg, seed=9, epoch=1, first=0, count=M, B=M, N=N, select=select, scale_shift=True, rotate=rotate,
                  order=order, num_cat=16)
    f = np.float32
    assert (ref["scale"] >= f(2.0 / 3.0)).all() and (ref["scale"] <= f(1.5)).all()
    assert (ref["shift"] >= f(-0.2)).all() and (ref["shift"] <= f(0.2)).all()
    assert len(np.unique(ref["scale"])) == 3 * M and len(np.unique(ref["shift"])) == 3 * M
    for b in range(M):
        Rb = ref["R"][b]
        assert abs(Rb @ Rb.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rb) - 1.0) < 1e-12
        if rotate == "z":
            assert np.array_equal(Rb[2], [0, 0, 1]) and np.array_equal(Rb[:, 2], [0, 0, 1])
        if rotate == "none":
            assert np.array_equal(Rb, np.eye(3))
        m = int(order[b])
        assert ref["y"][b] == label[m] and ref["onehot"][b].sum() == 1 and ref["onehot"][b, label[m]] == 1
        # un-transformed with its own parameters, the cloud is a rearrangement of pool points
        back = ((Rb.T @ ref["x"][b]).T - ref["shift"][b].astype(np.float64)) / ref["scale"][b].astype(np.float64)     # [N,3]
        src = data[m, :N] if select != "subset" else data[m]
        d = abs(back[:, None, :] - src[None, :, :].astype(np.float64)).max(-1)                                        # [N, |src|]
        hit = d.argmin(1)
        assert d.min(1).max() < 1e-6
        assert len(set(hit.tolist())) == N                                                                            # N DISTINCT points
        assert np.array_equal(hit, ref["perm"][b])
        if select == "first_shuffled":
            assert sorted(hit.tolist()) == list(range(N)) and not np.array_equal(hit, np.arange(N))
        if select == "first_ordered":
            assert np.array_equal(hit, np.arange(N))
        assert np.array_equal(ref["seg"][b], seg[m, ref["perm"][b]])
    assert len({tuple(p) for p in ref["perm"]}) == (1 if select == "first_ordered" else M)       # every cloud its own order


def test_fp32_evaluation_of_the_restatement_is_close_to_its_float64_one():
    data, label, seg = _pool()
    for rotate in ("none", "z", "so3"):
        ref = R.batch(data, label, seed=2, epoch=0, first=1, count=3, B=4, N=96, select="subset", scale_shift=True, rotate=rotate)
        params = np.zeros((4, 16), np.float32)
        params[:, 0:3], params[:, 3:6], params[:, 6:15] = ref["scale"], ref["shift"], ref["R"].reshape(4, 9).astype(np.float32)
        x32 = R.x_fp32(data, ref, params, True, rotate)
        assert x32.dtype == np.float32 and abs(x32 - ref["x"]).max() < 5e-6
        assert np.array_equal(x32[3], x32[0]) and not np.array_equal(x32[1], x32[0])             # slot 3 is past count: repeats slot 0


def test_slot_of_pool_point_zero_is_uniform():
    """Over 4096 clouds (seed 1234, epoch 3, g = 0..4095, N = 1024, first_shuffled) the slot pool point 0 lands in is uniform:
    chi-square over 16 equal bins against 56.49, the 1 - 1e-6 quantile at 15 degrees of freedom.  The 64-bit keys are unique."""
    N, G = 1024, 4096
    counts = np.zeros(16)
    for g in range(G):
        keys = R.point_keys(R.cloud_key(1234, 3, g), N)
        assert len(np.unique(keys)) == N
        slot = int((keys < keys[0]).sum())                   # rank of point 0's key = the output slot it lands in
        counts[slot * 16 // N] += 1
    expected = G / 16.0
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square %.2f" % chi2)
    assert chi2 < 56.49, chi2
    perm = R.point_order(R.cloud_key(1234, 3, 0), N, N, "first_shuffled")
    assert int(np.where(perm == 0)[0][0]) == int((R.point_keys(R.cloud_key(1234, 3, 0), N) < R.point_keys(R.cloud_key(1234, 3, 0), N)[0]).sum())
