"""Device-resident data sets and on-device batch assembly (svnet_amd/csrc/batch.hip).

What the reference does per sample on the host - `translate_pointcloud` and the point shuffle of its loaders (data.py:165-170,
192-198 ModelNet40, 284-294 ShapeNetPart, 327-337 ScanObjectNN), collate, copy to the device, rotate, permute
(main_cls_dgcnn.py:167-179) - is here ONE launch per batch: the whole pool lives on the device (ModelNet40 train is 242 MB) and a
batch is gathered and transformed straight into the fixed buffers a TrainStep / ForwardStep runs on.

    pool = DevicePool(data, label, device="cuda:0")                # data [M,P,3] float32 = np.asarray(h5['data']), label [M] or [M,1]
    loader = BatchLoader(pool, 32, 1024, select="first_shuffled", scale_shift=True, rotate="none", seed=1)
    step = TrainStep(model, inputs=(loader.x,), target=loader.y).capture()
    for epoch in range(E):
        loader.set_epoch(epoch)
        mean_loss = train_epoch(step, loader, optimizer)

Randomness is counter-based (splitmix64 `sm`, the one of svnet_amd/synth.py; all arithmetic on uint64, wrapping), never a stateful
generator: everything a cloud receives is a pure function of (seed, epoch, g), g = the cloud's position in the epoch order.  Batch
size, rank count, eager or replayed launches and a resume in mid-run cannot change what a sample looks like in an epoch, and the
host can restate a batch exactly (tests/loader_ref.py does).  The derivation:

    epoch_key = sm(sm(seed) ^ epoch)
    epoch order (shuffle=True): ascending order of the keys ((sm(order_key + i) >> 32) << 32) | i, i = 0..M-1,
                                order_key = sm(epoch_key ^ (2^64 - 1));  shuffle=False: 0..M-1
    cloud_key = sm(epoch_key ^ g)                                     = sm(sm(sm(seed) ^ epoch) ^ g)
    point order: ascending order of the keys ((sm(cloud_key + p) >> 16) << 16) | p, p = 0..S-1 (unique by construction: no tie
                 rule); S = N for "first_shuffled", S = P for "subset"; the first N of that order are taken, output slot n holds
                 pool point p_n.  "first_ordered": p_n = n.
    uniform u_j = (sm(cloud_key + 2^32 + j) >> 40) * 2^-24, exact in fp32, in [0, 1);  j = 0..2 scales, 3..5 shifts, 6..8 rotation
    scale_c = fl(LO + fl(SPAN * u_c)),     LO = fp32(2/3), SPAN = fp32(3/2 - 2/3)       (data.py:166)
    shift_c = fl(SLO + fl(SSPAN * u_3+c)), SLO = fp32(-0.2), SSPAN = fp32(0.4)          (data.py:167)
    coordinates: v_c = fl(fl(x_c * scale_c) + shift_c)                                  (only when scale_shift is on)
    rotation (only when rotate is "z" / "so3"), all in fp32, sinpi / cospi of the exact argument 2u:
        "z":   s, c = sin, cos(2 pi u_6);  R = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        "so3": a = sqrt(1 - u_6), b = sqrt(u_6); unit quaternion (w, i, j, k) = (b cos 2 pi u_8, a sin 2 pi u_7, a cos 2 pi u_7,
               b sin 2 pi u_8) - uniform on S^3 (Shoemake), hence R uniform on SO(3); R = the matrix of train.rotate_clouds:
               [[1-2(jj+kk), 2(ij-kw), 2(ik+jw)], [2(ij+kw), 1-2(ii+kk), 2(jk-iw)], [2(ik-jw), 2(jk+iw), 1-2(ii+jj)]]
        out_r = fl(fl(fl(R_r0 * v_0) + fl(R_r1 * v_1)) + fl(R_r2 * v_2))                (R x, as train.rotate_clouds' bmm)
    Every operation is a single-rounded fp32 operation, never contracted into an fma.  The kernel writes the 3 scales, 3 shifts and
    9 rotation entries it used into `params` [B,16] (no augmentation: 1, 0, identity; those operations are then skipped, not
    multiplied through).

Attributes.  A pool may carry A more floats per point, `attr` [M,P,A] (the reference's ModelNet40_v2(normal_channel=True), data.py:203-256,
keeps six columns per point, its S3DIS set nine).  They arrive in `loader.points` [B,A,N], channel-first as the set-abstraction levels
take `points`, filled by the same launch as `loader.x`: slot n of cloud b holds the attributes of the pool point x[b,:,n] came from.

    pool = DevicePool(data, label, attr=normals_and_colours, attr_vectors=1, device="cuda:0")       # attr [M,P,6]: a normal, then r g b
    loader = BatchLoader(pool, 32, 1024, select="first_shuffled", scale_shift=True, rotate="so3", seed=1)
    step = TrainStep(model, inputs=(loader.x, loader.points), target=loader.y)

    The first `attr_vectors` groups of three channels are direction vectors (unit normals), the other channels scalars.
    scalar channels: the pool's bits (-0 stays -0), whatever the augmentation.
    direction group (n_0, n_1, n_2): the coordinates undergo x' = R (S x) + shift with S = diag(scale); a normal transforms with the
        inverse transpose of the linear part, R S^-1, the shift does nothing, and its length is restored:
        scale_shift on:   q_c = fl(n_c / scale_c);  l2 = fl(fl(fl(q_0 q_0) + fl(q_1 q_1)) + fl(q_2 q_2));  l = fl(sqrt(l2));
                          if l > 0: q_c = fl(q_c / l)  (a zero or underflowing vector stays as the first division left it)
        scale_shift off:  q = n, bit for bit
        rotate "z" / "so3": out_r = fl(fl(fl(R_r0 q_0) + fl(R_r1 q_1)) + fl(R_r2 q_2)), R the nine entries written to `params`;
        rotate "none":      out = q
    Single-rounded fp32 operations as above, division and square root correctly rounded.  With scale_shift on a direction group
    therefore comes out at UNIT length whatever length it had in the pool - which is what a normal is; with it off, lengths are kept
    (a rotation changes them by rounding only).  No further random numbers are drawn and `params` keeps its layout.  The reference
    never augments a six-column cloud, so this rule is the project's own; tests/loader_attr_ref.py restates it, and checks that the
    result stays perpendicular to the transformed surface.  Non-finite attributes give unspecified values.
    resample_fps carries the attributes: sampling and pc_normalize look at the coordinates only (data.py:241-248 normalises
    point_set[:, 0:3]; a translation and an isotropic scale leave a normal as it is), the new attr[m,n,:] = attr[m, fps_index[m,n], :].

Uniformly resampled pools (the reference's ModelNet40_v2(uniform=True), data.py:203-256: ~10 000-point clouds reduced to num_points
by `farthest_point_sample`, models/utils/pointnet_util.py:63-84, then `pc_normalize`, data.py:15-20) are made once, on the device
(svnet_amd/csrc/fps.hip), and the result is an ordinary pool:

    big = DevicePool(data10k, label, device="cuda:0")                   # [M,10000,3]: past the loader's 8192-point limit
    pool = big.resample_fps(1024, seed=0, normalize=True)               # [M,1024,3]; pool.fps_index [M,1024] says which points

    for one cloud xyz [P,3], a start index s and npoint <= P (all fp32, each operation rounded once, never an fma):
        mind[p] = fp32(1e10);  f = s
        for i in 0 .. npoint-1:  idx[i] = f;  d_c = fl(xyz[p,c] - xyz[f,c]);  dist = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))
                                 (the point-set helpers' one distance: svnet_amd/csrc/pointset.h)
                                 mind[p] = dist < mind[p] ? dist : mind[p];  f = the smallest p with mind[p] == max_p mind[p]
    which is the reference's loop with its `torch.randint` start made an input (default: fps_start, counter-based like everything
    above): given the start, the index list equals the reference's CPU result bit for bit.  Coordinates must be finite.
    normalize: c = the float64 mean of the N selected points (fixed summation order) rounded once to fp32, d = fl(p - c),
        m = max_n sqrt(fl(fl(d_0 d_0 + d_1 d_1) + d_2 d_2)), out = fl(d / m): single-rounded fp32, the same bits on every run (numpy's
        float32 mean rounds differently: close to the reference's output, not bit-identical to it).

There is no CPU fallback: a pool that is not on a HIP device raises.
"""
import ctypes

import numpy as np
import torch

from . import _call, _lib, _pointset, synth

SELECT_MODES = {m: _lib.DEFINES["SVNET_BATCH_" + m.upper()] for m in ("first_shuffled", "subset", "first_ordered")}
MAX_ATTR = _lib.DEFINES["SVNET_BATCH_MAX_ATTR"]
ROTATE_MODES = {m: _lib.DEFINES["SVNET_BATCH_ROTATE_" + (m or "none").upper()] for m in ("none", None, "z", "so3")}

_U64 = np.uint64


def _sm(x):
    return synth._splitmix64(np.asarray(x, dtype=np.uint64))


def _epoch_key(seed, epoch):
    return _sm(_sm(_U64(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ _U64(int(epoch) & 0xFFFFFFFFFFFFFFFF))


def epoch_order(seed, epoch, M):
    """The epoch's sample order: a permutation of 0..M-1 as int64 numpy (host side, once per epoch; see the module docstring)."""
    M = int(M)
    if not 0 < M < (1 << 32):
        raise ValueError("epoch_order: M = %d outside 1 .. 2^32 - 1" % M)
    order_key = _sm(_epoch_key(seed, epoch) ^ _U64(0xFFFFFFFFFFFFFFFF))
    i = np.arange(M, dtype=np.uint64)
    with np.errstate(over="ignore"):
        keys = ((_sm(order_key + i) >> _U64(32)) << _U64(32)) | i
    return np.argsort(keys, kind="stable").astype(np.int64)


def fps_start(seed, M, P):
    """The default start index of cloud m = 0..M-1 for farthest point sampling: sm(sm(seed) ^ m) mod P as int64 numpy; a pure function
    of (seed, m) (the reference draws it with torch.randint, pointnet_util.py:75)."""
    M, P = int(M), int(P)
    if M < 1 or P < 1:
        raise ValueError("fps_start: M = %d, P = %d must be positive" % (M, P))
    m = np.arange(M, dtype=np.uint64)
    return (_sm(_sm(_U64(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ m) % _U64(P)).astype(np.int64)


def farthest_point_sample(xyz, npoint, start):
    """Farthest point sampling (models/utils/pointnet_util.py:63 farthest_point_sample, same return convention): xyz [B,P,3] float32
    on a HIP device, start [B] int64 (the first centroid of every cloud, which the reference draws at random) -> [B,npoint] int64.
    Given the start the result equals the reference's CPU result bit for bit (module docstring).  A preparation-time call: the start
    range is checked with one device reduction and one synchronisation before the launch."""
    if not isinstance(xyz, torch.Tensor) or not isinstance(start, torch.Tensor):
        raise TypeError("farthest_point_sample: xyz and start must be tensors")
    _call.hip(xyz, start)
    if xyz.dtype != torch.float32 or start.dtype != torch.int64:
        raise TypeError("farthest_point_sample: xyz must be float32 and start int64, got %s and %s" % (xyz.dtype, start.dtype))
    B, P = _pointset.check_cloud("farthest_point_sample", "xyz", xyz, "P")
    npoint = int(npoint)
    if tuple(start.shape) != (B,):
        raise ValueError("farthest_point_sample: start must be [B] = [%d], got %s" % (B, tuple(start.shape)))
    if not xyz.is_contiguous() or not start.is_contiguous():
        raise ValueError("farthest_point_sample: xyz and start must be contiguous")
    if start.device != xyz.device:
        raise ValueError("farthest_point_sample: xyz on %s, start on %s" % (xyz.device, start.device))
    _pointset.fps_supported("farthest_point_sample", "P", P, npoint)
    lo, hi = (int(v) for v in torch.aminmax(start))
    if lo < 0 or hi >= P:
        raise ValueError("farthest_point_sample: start outside 0 .. P-1 = %d (min %d, max %d)" % (P - 1, lo, hi))
    idx = torch.empty(B, npoint, dtype=torch.int64, device=xyz.device)
    _pointset.fps_launch(xyz, B, P, npoint, start, idx)
    return idx


def _as_tensor(a, dtype, name):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != dtype:
        raise TypeError("DevicePool: %s must be %s, got %s" % (name, dtype, t.dtype))
    return t


class DevicePool:
    """A whole data set on the device: data [M,P,3] float32 (point-major, as the HDF5 files hold it: `np.asarray(h5['data'])` is what
    goes in), label [M] or [M,1] int64, optional seg [M,P] int64, optional attr [M,P,A] float32 with 1 <= A <= 32 whose first
    `attr_vectors` groups of three channels are direction vectors (module docstring, "Attributes"); .A is 0 without attributes.
    numpy arrays or tensors; moved to `device` once."""

    def __init__(self, data, label, seg=None, attr=None, attr_vectors=0, device="cuda:0"):
        data = _as_tensor(data, torch.float32, "data")
        label = _as_tensor(label, torch.int64, "label")
        if data.dim() != 3 or data.shape[2] != 3 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError("DevicePool: data must be [M,P,3], got %s" % (tuple(data.shape),))
        M, P = int(data.shape[0]), int(data.shape[1])
        if tuple(label.shape) not in ((M,), (M, 1)):
            raise ValueError("DevicePool: label must be [M] or [M,1] with M = %d, got %s" % (M, tuple(label.shape)))
        if seg is not None:
            seg = _as_tensor(seg, torch.int64, "seg")
            if tuple(seg.shape) != (M, P):
                raise ValueError("DevicePool: seg must be [M,P] = %s, got %s" % ((M, P), tuple(seg.shape)))
        A, attr_vectors = 0, int(attr_vectors)
        if attr is not None:
            attr = _as_tensor(attr, torch.float32, "attr")
            if attr.dim() != 3 or tuple(attr.shape[:2]) != (M, P) or not 1 <= attr.shape[2] <= MAX_ATTR:
                raise ValueError("DevicePool: attr must be [M,P,A] = [%d,%d,1 .. %d], got %s" % (M, P, MAX_ATTR, tuple(attr.shape)))
            A = int(attr.shape[2])
        if not 0 <= 3 * attr_vectors <= A:
            raise ValueError("DevicePool: attr_vectors = %d: 3 x it must lie in 0 .. A = %d" % (attr_vectors, A))
        device = _pointset.hip_device("DevicePool", device)
        self.M, self.P, self.device = M, P, device
        self.A, self.attr_vectors = A, attr_vectors
        self.attr = None if attr is None else attr.to(device).contiguous()
        self.data = data.to(device).contiguous()
        self.label = label.reshape(M).to(device).contiguous()
        self.seg = None if seg is None else seg.to(device).contiguous()

    def resample_fps(self, num_points, *, start=None, seed=0, normalize=False):
        """A new pool [M,num_points,3] on the same device: every cloud reduced to `num_points` by farthest point sampling, optionally
        followed by pc_normalize (module docstring) - how a pool of more than 8192 points per cloud gets under the BatchLoader's limit.
        `start` [M] int64 (numpy or tensor) is the first centroid of every cloud; None: fps_start(seed, M, P).  `label` is shared,
        `seg` and `attr` are gathered (attr[m,n,:] = attr[m, fps_index[m,n], :] bit for bit; sampling and normalisation look at the
        coordinates only), and `.fps_index` [M,num_points] keeps which point of the source every point is."""
        N = int(num_points)
        if start is None:
            start = fps_start(seed, self.M, self.P)
        start = _as_tensor(start, torch.int64, "start").to(self.device).contiguous()
        idx = farthest_point_sample(self.data, N, start)
        new = object.__new__(DevicePool)
        new.M, new.P, new.device = self.M, N, self.device
        new.data = torch.empty(self.M, N, 3, dtype=torch.float32, device=self.device)
        new.label = self.label
        new.seg = None if self.seg is None else torch.empty(self.M, N, dtype=torch.int64, device=self.device)
        new.A, new.attr_vectors = self.A, self.attr_vectors
        new.attr = None if self.attr is None else torch.empty(self.M, N, self.A, dtype=torch.float32, device=self.device)
        new.fps_index = idx
        with torch.cuda.device(self.device):
            _lib.call("svnet_pool_gather_f32", _call.p(self.data), _call.p(self.seg), _call.p(idx), self.M, self.P, N,
                      int(bool(normalize)), _call.p(new.data), _call.p(new.seg), _call.stream())
            if self.attr is not None:
                _lib.call("svnet_pool_gather_attr_f32", _call.p(self.attr), _call.p(idx), self.M, self.P, N, self.A, _call.p(new.attr),
                          _call.stream())
        return new

    def source_points(self, source_pool):
        """[M,N,3]: this resampled pool's points in the frame of `source_pool`, the pool it was made from by resample_fps
        (svnet_amd/propagate.py source_points: source_pool.data gathered by fps_index; raises without an fps_index)."""
        from .propagate import source_points
        return source_points(self, source_pool)

    @staticmethod
    def synthetic_arrays(seed, M, P, num_class, num_part=None):
        """(data, label, seg or None) of a synthetic pool as numpy: the clouds of synth.cloud_batch, point-major."""
        data = np.ascontiguousarray(synth.cloud_batch(seed, 0, 0, M, P).transpose(0, 2, 1))
        label = synth.class_labels(seed, 0, 0, M, num_class)
        seg = None if num_part is None else synth.seg_labels(seed, 0, 0, M, P, num_part)
        return data, label, seg

    @classmethod
    def synthetic(cls, seed, M, P, num_class, num_part=None, device="cuda:0"):
        """A pool of M synthetic clouds of P points (tests and tools): labels < num_class, per-point labels < num_part if given."""
        return cls(*cls.synthetic_arrays(seed, M, P, num_class, num_part), device=device)


def steps_per_epoch(M, batch_size, world=1, drop_last=True):
    """Steps every rank takes per epoch: rank r fills its batch of step s from positions (s * world + r) * B + b of the epoch order."""
    per_step = int(batch_size) * int(world)
    return int(M) // per_step if drop_last else -(-int(M) // per_step)


def batch_span(M, batch_size, step, rank=0, world=1):
    """(first, count) of `rank`'s batch at `step`: positions first .. first + count - 1 of the epoch order (count 0: nothing left)."""
    first = (int(step) * int(world) + int(rank)) * int(batch_size)
    return first, max(0, min(int(batch_size), int(M) - first))


class BatchLoader:
    """Fills fixed device buffers with one batch per `load(step)`, one launch each (see the module docstring).

    .x [B,3,N] float32 (the models' input), .y [B] int64, .seg [B,N] int64 (pools with seg), .onehot [B,num_cat] float32 (when
    num_cat is given: the one-hot of the label, the part-seg models' second input), .params [B,16] float32 (the augmentation used),
    .points [B,A,N] float32 (pools with attr, else None: the per-point attributes in .x's point order, direction vectors transformed
    with the coordinates - with scale_shift on they come out at unit length; module docstring, "Attributes").
    select: "first_shuffled" (ModelNet40 / ShapeNetPart training), "subset" (ScanObjectNN), "first_ordered" (every test partition).
    """

    def __init__(self, pool, batch_size, num_points, *, select, scale_shift, rotate, shuffle=True, drop_last=True, seed,
                 rank=0, world=1, num_cat=None):
        if not isinstance(pool, DevicePool):
            raise TypeError("BatchLoader: pool must be a DevicePool")
        _call.hip(pool.data, pool.label, pool.seg, pool.attr)
        if select not in SELECT_MODES:
            raise ValueError("BatchLoader: select must be one of %r" % sorted(SELECT_MODES))
        if rotate not in ROTATE_MODES:
            raise ValueError("BatchLoader: rotate must be 'none', 'z' or 'so3'")
        B, N = int(batch_size), int(num_points)
        if B < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("BatchLoader: batch_size %d, rank %d of %d" % (B, rank, world))
        if N < 1 or N > pool.P:
            raise ValueError("BatchLoader: num_points %d outside 1 .. P = %d" % (N, pool.P))
        if not 0 <= int(seed) < (1 << 63):
            raise ValueError("BatchLoader: seed must be in 0 .. 2^63 - 1")
        self.select_mode = SELECT_MODES[select]
        if not _lib.lib().svnet_batch_supported(pool.P, N, self.select_mode):
            raise _lib.SvnetHipError("BatchLoader: P = %d, N = %d, select = %r is not supported (the point keys of a cloud must fit "
                                     "64 KiB of LDS: at most 8192)" % (pool.P, N, select))
        self.pool, self.B, self.N = pool, B, N
        self.scale_shift, self.rotate = int(bool(scale_shift)), ROTATE_MODES[rotate]
        self.shuffle, self.drop_last, self.seed = bool(shuffle), bool(drop_last), int(seed)
        self.rank, self.world = int(rank), int(world)
        dev = pool.device
        self.x = torch.zeros(B, 3, N, dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.int64, device=dev)
        self.seg = None if pool.seg is None else torch.zeros(B, N, dtype=torch.int64, device=dev)
        self.num_cat = None if num_cat is None else int(num_cat)
        self.onehot = None if num_cat is None else torch.zeros(B, self.num_cat, dtype=torch.float32, device=dev)
        self.params = torch.zeros(B, 16, dtype=torch.float32, device=dev)
        self.points = None if pool.attr is None else torch.zeros(B, pool.A, N, dtype=torch.float32, device=dev)
        self.order = torch.empty(pool.M, dtype=torch.int64, device=dev)
        self.epoch = None
        self._desc = _lib.BatchDesc()
        d = self._desc
        d.data, d.label, d.seg, d.order = _call.p(pool.data), _call.p(pool.label), _call.p(pool.seg), _call.p(self.order)
        d.M, d.P, d.L, d.B, d.N = pool.M, pool.P, pool.M, B, N
        d.seed = self.seed
        d.select_mode, d.scale_shift, d.rotate = self.select_mode, self.scale_shift, self.rotate
        d.num_cat = self.num_cat or 0
        d.x, d.y, d.seg_out, d.onehot, d.params = _call.p(self.x), _call.p(self.y), _call.p(self.seg), _call.p(self.onehot), _call.p(self.params)
        d.attr, d.A, d.attr_vectors, d.attr_out = _call.p(pool.attr), pool.A, pool.attr_vectors, _call.p(self.points)
        self.set_epoch(0)

    def set_epoch(self, epoch):
        """Fix the epoch: its sample order (one host argsort of M keys, one small copy to the device) and its augmentation stream."""
        if not 0 <= int(epoch) < (1 << 63):
            raise ValueError("BatchLoader.set_epoch: epoch must be in 0 .. 2^63 - 1")
        self.epoch = int(epoch)
        order = epoch_order(self.seed, self.epoch, self.pool.M) if self.shuffle else np.arange(self.pool.M, dtype=np.int64)
        self.order.copy_(torch.from_numpy(order))       # (stream-ordered on the current stream: behind the previous epoch's launches)
        self._desc.epoch = self.epoch

    def __len__(self):
        return steps_per_epoch(self.pool.M, self.B, self.world, self.drop_last)

    def span(self, step):
        return batch_span(self.pool.M, self.B, step, self.rank, self.world)

    def load(self, step):
        """Enqueue the assembly of this rank's batch of `step` on the current stream; returns the number of valid clouds (slots past
        it repeat slot 0; 0 = this rank has no cloud left at this step and nothing was launched)."""
        if not 0 <= int(step) < len(self):
            raise IndexError("BatchLoader.load: step %d outside 0 .. %d" % (step, len(self) - 1))
        first, count = self.span(step)
        if count == 0:
            return 0
        self._desc.first, self._desc.count = first, count
        _lib.call("svnet_batch_assemble_f32", ctypes.byref(self._desc), _call.stream())
        return count
