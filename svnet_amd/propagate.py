"""Feature propagation from sampled points to the dense cloud they were sampled from (svnet_amd/csrc/propagate.hip).

`DevicePool.resample_fps` (svnet_amd/data.py) reduces dense clouds to the 1024 or 2048 points a model trains and predicts on.  This
module carries a prediction back: PointNet++'s inverse-squared-distance interpolation over the three nearest sampled points, the
reference's `PointNetFeaturePropagation.forward` (models/utils/pointnet_util.py:281-308, via `square_distance` and `index_points`)
without its MLP - farthest point sampling's counterpart from the same file.

    dense = DevicePool(data10k, label, seg, device="cuda:0")            # [M,10000,3]
    pool = dense.resample_fps(2048, seed=0, normalize=True)             # what the model sees
    ref = source_points(pool, dense)                                    # [M,2048,3]: the sampled points in `dense`'s frame
    logits_dense = propagate(dense.data[m0:m1], ref[m0:m1], logits)     # [B,50,2048] -> [B,50,10000]
    result = train.evaluate_dense(fwd_step, loader, metrics, dense)     # the whole evaluation pass, shape IoU of the CLOUDS

The contract, for one cloud: queries q [P,3], sampled points r [N,3], features f [D,N] (channel-first, as the part-seg models'
[B,num_part,N] logits lie), all fp32.  Every operation is rounded once and never contracted into an fma; fl() is rounding to fp32.

    distances   d_c = fl(q[p,c] - r[n,c]);   dist[p,n] = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))
                The point-set helpers' one distance, the difference form: never negative, exactly 0 at a coincident point - which
                every sampled point is after resample_fps (svnet_amd/csrc/pointset.h states it and why the reference's expanded form
                -2 q.r + |q|^2 + |r|^2 is not copied).
    neighbours  the K = min(3, N) smallest dist[p,:], ascending, the lower index first among equals: idx [P,3] int64 and
                dist3 [P,3] fp32.  Slots past K (N < 3 only) hold index 0, dist3 = +inf and weight 0.  Indices are always inside
                [0, N), also when a coordinate is NaN or infinite (a NaN or +inf distance is never taken; its slot stays as a slot
                past K): results are then unspecified but in range.
    weights     rec_j = fl(1 / fl(dist3_j + fp32(1e-8)));   s = fl(fl(rec_0 + rec_1) + rec_2);   w_j = fl(rec_j / s)
                Both divisions are correctly rounded.
    values      out[d,p] = fl(fl(fl(f[d,i_0] w_0) + fl(f[d,i_1] w_1)) + fl(f[d,i_2] w_2))
                N = 1 gives w_0 = 1 and out = f[d,0], the reference's `S == 1` branch (finite features: 0 * inf is NaN).

On coordinates whose squares and products are exact in fp32 the two distance forms agree bit for bit, and there the whole contract
equals the reference's CPU result bit for bit (tests/golden/propagate.npz; tests/propagate_ref.py restates the contract in numpy).

Gradients: `feat` may require grad in three_interpolate() and propagate(); the call then goes through a torch.autograd.Function
whose backward is three_interpolate_backward() (svnet_amd/csrc/pointset_grad.hip), the adjoint of `values` above:

    backward    with the edges e = 3 p + j that point to n (idx clamped as the forward clamps it) in ascending e, e_1 < e_2 < ...,
                and t_i = fl(dout[d,p_i] w[p_i,j_i]):   dfeat[d,n] = fl(fl(fl(t_1 + t_2) + t_3) + ...); one term gives t_1, no term
                +0.  A fixed order and no float atomic: two runs give the same bits (tests/pointset_grad_ref.py restates it).

Coordinates are data: no gradient goes to query, ref or weight, and a coordinate, weight or index that requires grad is refused, as
is `out=` beside a feat that requires grad.  The classes stay forward only.  There is no CPU fallback: tensors that are not on a
HIP device raise.  Limits: 1 <= N <= 32768 (the k-NN's limit), P >= 1, D >= 1, B * ceil(P / 256) <= 2^31 - 1.
"""
import torch

from . import _call, _lib, _pointset

_WHAT = "the propagation"        # in the messages of _pointset.check_tensors


def tile():
    """Sampled points per LDS tile of the three_nn kernel: the N past which its candidate loop takes another tile."""
    return int(_lib.lib().svnet_propagate_tile())


def _supported(name, P, N, D):
    if not _lib.lib().svnet_propagate_supported(P, N, D):
        raise _lib.SvnetHipError("%s: P = %d, N = %d, D = %d is not supported (P >= 1, D >= 1, 1 <= N <= %d)" % (name, P, N, D, _pointset.MAX_N))


def _nn_shapes(name, query, ref):
    return _pointset.check_cloud_pair(name, ("query", "ref"), query, ref, "PN")


def _nn_launch(query, ref, B, P, N, idx, dist3, weight):
    with torch.cuda.device(query.device):
        _lib.call("svnet_three_nn_f32", _call.p(query), _call.p(ref), B, P, N, _call.p(idx), _call.p(dist3), _call.p(weight), _call.stream())


def _interp_launch(feat, idx, weight, B, D, N, P, out):
    with torch.cuda.device(feat.device):
        _lib.call("svnet_three_interpolate_f32", _call.p(feat), _call.p(idx), _call.p(weight), B, D, N, P, _call.p(out), _call.stream())


def three_nn(query, ref):
    """query [B,P,3], ref [B,N,3] float32 on a HIP device -> (idx [B,P,3] int64, dist3 [B,P,3], weight [B,P,3]): the three nearest
    `ref` points of every query point and their interpolation weights (module docstring).  One launch, no host read; no gradient."""
    _pointset.check_tensors("three_nn", {"query": query, "ref": ref}, (torch.float32, torch.float32), _WHAT)
    B, P, N = _nn_shapes("three_nn", query, ref)
    _call.hip(query, ref)
    _supported("three_nn", P, N, 1)
    idx = torch.empty(B, P, 3, dtype=torch.int64, device=query.device)
    dist3 = torch.empty(B, P, 3, dtype=torch.float32, device=query.device)
    weight = torch.empty(B, P, 3, dtype=torch.float32, device=query.device)
    _nn_launch(query, ref, B, P, N, idx, dist3, weight)
    return idx, dist3, weight


def _interp_shapes(name, feat, idx, weight):
    if feat.dim() != 3 or feat.shape[0] < 1:
        raise ValueError("%s: feat must be [B,D,N], got %s" % (name, tuple(feat.shape)))
    if idx.dim() != 3 or idx.shape[2] != 3 or idx.shape[0] != feat.shape[0] or tuple(weight.shape) != tuple(idx.shape):
        raise ValueError("%s: idx and weight must be [B,P,3] with B = %d, got %s and %s"
                         % (name, feat.shape[0], tuple(idx.shape), tuple(weight.shape)))
    return int(feat.shape[0]), int(feat.shape[1]), int(feat.shape[2]), int(idx.shape[1])


def _out_buffer(name, out, feat, B, D, P):
    if out is None:
        return torch.empty(B, D, P, dtype=torch.float32, device=feat.device)
    _pointset.check_out(name, {"feat": feat}, out, "[B,D,P]", (B, D, P), _WHAT)
    return out


def _no_out_with_grad(name, arg, out):
    if out is not None:
        raise ValueError("%s: out= beside a %s that requires grad - autograd owns the result of a differentiable call" % (name, arg))


class _Interpolate(torch.autograd.Function):
    """three_interpolate for a feat that requires grad: the forward launch, and three_interpolate_backward as its backward (current
    stream, no host read: capturable).  idx and weight get no gradient."""

    @staticmethod
    def forward(ctx, feat, idx, weight):
        B, D, N, P = _interp_shapes("three_interpolate", feat, idx, weight)
        out = torch.empty(B, D, P, dtype=torch.float32, device=feat.device)
        _interp_launch(feat, idx, weight, B, D, N, P, out)
        ctx.save_for_backward(idx, weight)
        ctx.N = N
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        idx, weight = ctx.saved_tensors
        return three_interpolate_backward(dout.contiguous(), idx, weight, ctx.N), None, None


def three_interpolate(feat, idx, weight, out=None):
    """feat [B,D,N] float32, idx [B,P,3] int64, weight [B,P,3] float32 -> [B,D,P]: out[b,d,p] = sum_j feat[b,d,idx[b,p,j]] weight[b,p,j]
    in the contract's order.  An index outside [0, N) is clamped into it.  One launch, no host read.  feat may require grad (module
    docstring); idx and weight may not."""
    grad = _pointset.check_tensors("three_interpolate", {"feat": feat, "idx": idx, "weight": weight},
                                   (torch.float32, torch.int64, torch.float32), _WHAT, grad=("feat",))
    B, D, N, P = _interp_shapes("three_interpolate", feat, idx, weight)
    _call.hip(feat, idx, weight)
    _supported("three_interpolate", P, N, D)
    if grad:
        _no_out_with_grad("three_interpolate", "feat", out)
        return _Interpolate.apply(feat, idx, weight)
    out = _out_buffer("three_interpolate", out, feat, B, D, P)
    _interp_launch(feat, idx, weight, B, D, N, P, out)
    return out


def three_interpolate_backward(dout, idx, weight, N, out=None):
    """The gradient of three_interpolate with respect to feat: dout [B,D,P] float32, idx [B,P,3] int64, weight [B,P,3] float32 ->
    dfeat [B,D,N], the ordered sums of the module docstring.  Two launches on the current stream (the reverse lists of idx, the
    sums), no host read; `out` lets a caller keep a fixed buffer.  Every element of dfeat is written, an empty list as +0."""
    _pointset.check_tensors("three_interpolate_backward", {"dout": dout, "idx": idx, "weight": weight},
                            (torch.float32, torch.int64, torch.float32), _WHAT)
    B, D, P, _ = _interp_shapes("three_interpolate_backward", dout, idx, weight)
    N = int(N)
    if idx.shape[1] != P:
        raise ValueError("three_interpolate_backward: dout must be [B,D,P] with P = %d, got %s" % (idx.shape[1], tuple(dout.shape)))
    _call.hip(dout, idx, weight)
    _supported("three_interpolate_backward", P, N, D)
    _pointset.reverse_supported("three_interpolate_backward", P, 3, N)
    if out is None:
        out = torch.empty(B, D, N, dtype=torch.float32, device=dout.device)
    else:
        _pointset.check_out("three_interpolate_backward", {"dout": dout}, out, "[B,D,N]", (B, D, N), _WHAT)
    rev_start, rev_edge = _pointset.reverse_lists(idx, N)
    with torch.cuda.device(dout.device):
        _lib.call("svnet_three_interpolate_bwd_f32", _call.p(dout), _call.p(weight), _call.p(rev_start), _call.p(rev_edge), B, D, N, P,
                  _call.p(out), _call.stream())
    return out


def propagate(query, ref, feat, out=None):
    """three_nn(query, ref) then three_interpolate(feat, ...): feat [B,D,N] at the points ref [B,N,3] -> [B,D,P] at query [B,P,3].
    Two launches on the current stream, no host read and no synchronisation, so it can be captured in a HIP graph; `out` lets a
    caller keep a fixed buffer.  feat may require grad (module docstring); query and ref may not."""
    grad = _pointset.check_tensors("propagate", {"query": query, "ref": ref, "feat": feat}, (torch.float32,) * 3, _WHAT, grad=("feat",))
    B, P, N = _nn_shapes("propagate", query, ref)
    if feat.dim() != 3 or feat.shape[0] != B or feat.shape[2] != N:
        raise ValueError("propagate: feat must be [B,D,N] with B = %d, N = %d, got %s" % (B, N, tuple(feat.shape)))
    D = int(feat.shape[1])
    _call.hip(query, ref, feat)
    _supported("propagate", P, N, D)
    if grad:
        _no_out_with_grad("propagate", "feat", out)
    else:
        out = _out_buffer("propagate", out, feat, B, D, P)
    idx = torch.empty(B, P, 3, dtype=torch.int64, device=query.device)
    dist3 = torch.empty(B, P, 3, dtype=torch.float32, device=query.device)
    weight = torch.empty(B, P, 3, dtype=torch.float32, device=query.device)
    _nn_launch(query, ref, B, P, N, idx, dist3, weight)
    if grad:
        return _Interpolate.apply(feat, idx, weight)
    _interp_launch(feat, idx, weight, B, D, N, P, out)
    return out


class Propagator:
    """propagate() on buffers allocated once: the neighbour and weight buffers for up to B clouds of P query points and the output
    [B,D,P].  run(query, ref, feat) takes the first `count` clouds of each and returns out[:count]; nothing is allocated per call."""

    def __init__(self, B, D, N, P, device):
        device = _pointset.hip_device("Propagator", device)
        self.B, self.D, self.N, self.P = int(B), int(D), int(N), int(P)
        if self.B < 1:
            raise ValueError("Propagator: B = %d < 1" % self.B)
        _supported("Propagator", self.P, self.N, self.D)
        self.idx = torch.empty(self.B, self.P, 3, dtype=torch.int64, device=device)
        self.dist3 = torch.empty(self.B, self.P, 3, dtype=torch.float32, device=device)
        self.weight = torch.empty(self.B, self.P, 3, dtype=torch.float32, device=device)
        self.out = torch.empty(self.B, self.D, self.P, dtype=torch.float32, device=device)

    def run(self, query, ref, feat):
        _pointset.check_tensors("Propagator.run", {"query": query, "ref": ref, "feat": feat}, (torch.float32,) * 3, _WHAT)
        count, P, N = _nn_shapes("Propagator.run", query, ref)
        _call.hip(query, ref, feat)
        if count > self.B or (P, N) != (self.P, self.N) or tuple(feat.shape) != (count, self.D, N) or query.device != self.out.device:
            raise ValueError("Propagator.run: query %s, ref %s, feat %s do not fit B <= %d, D %d, N %d, P %d on %s"
                             % (tuple(query.shape), tuple(ref.shape), tuple(feat.shape), self.B, self.D, self.N, self.P, self.out.device))
        _nn_launch(query, ref, count, P, N, self.idx, self.dist3, self.weight)
        _interp_launch(feat, self.idx, self.weight, count, self.D, N, P, self.out)
        return self.out[:count]


def source_points(pool, source_pool):
    """The [M,N,3] coordinates of a resampled pool's points in the frame of the pool it came from: source_pool.data gathered by
    pool.fps_index.  (`normalize=True` moved the sampled pool's own coordinates, so pool.data is not that.)  Raises when `pool` has
    no fps_index or the sizes do not match.  A preparation-time call: the index range is checked with one device reduction and one
    synchronisation."""
    from .data import DevicePool
    if not isinstance(pool, DevicePool) or not isinstance(source_pool, DevicePool):
        raise TypeError("source_points: pool and source_pool must be DevicePools")
    index = getattr(pool, "fps_index", None)
    if index is None:
        raise ValueError("source_points: the pool has no fps_index - it was not made by DevicePool.resample_fps")
    if pool.M != source_pool.M or tuple(index.shape) != (pool.M, pool.P) or pool.P > source_pool.P:
        raise ValueError("source_points: a pool of %d clouds of %d points (fps_index %s) was not sampled from a pool of %d clouds of %d points"
                         % (pool.M, pool.P, tuple(index.shape), source_pool.M, source_pool.P))
    if index.device != source_pool.data.device:
        raise ValueError("source_points: fps_index on %s, the source pool on %s" % (index.device, source_pool.data.device))
    lo, hi = (int(v) for v in torch.aminmax(index))
    if lo < 0 or hi >= source_pool.P:
        raise ValueError("source_points: fps_index outside 0 .. P-1 = %d (min %d, max %d)" % (source_pool.P - 1, lo, hi))
    return _pointset.gather_rows(source_pool.data, index).contiguous()
