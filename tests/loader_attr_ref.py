"""Helper (not a test): a numpy restatement of the per-point attributes of one assembled batch (`loader.points` [B,A,N]), written
from the "Attributes" paragraph of svnet_amd/data.py's docstring - not from the kernel.  The keys, the point order and the
parameters are tests/loader_ref.py's (`ref = loader_ref.batch(...)`); nothing of them is restated here.

    normal_f64(n, scale, R, scale_shift) [...,3]       the rule for one direction vector in float64: R (S^-1 n) / |S^-1 n|
    points_f64(attr, ref, attr_vectors, scale_shift)   [B,A,N] float64 with ref["scale"] and ref["R"]
    points_fp32(attr, ref, params, attr_vectors, scale_shift, rotate) [B,A,N] float32: the same in fp32, operation by operation, with a
        given `params` [B,16] (the device's own): what the kernel's points must equal bit for bit.

FP32_BOUND: |points_fp32 - points_f64| for a direction component when both use the same scales and the fp32 rounding of the same R.
Count the single-rounded operations behind one output component, u = 2^-24 the unit roundoff of round-to-nearest fp32:
    R_rc rounded to fp32 (1), q_c = n_c / scale_c (1), the three products and two sums of l2 (5), the square root (1), q_c / l (1),
    the three products and two sums of the rotation (5): 14 operations.
No intermediate exceeds 3/2 in magnitude where its error enters the result absolutely: |n| <= 1, 2/3 <= scale <= 3/2, so |q_c| <= 3/2
before the normalisation and <= 1 after it, |R_rc| <= 1, and a row of R times a unit vector is <= 1 (l2 <= 9/4 enters only through
its RELATIVE error, which the all-positive sum keeps at 3u and the root halves).  To first order the error is therefore at most
14 operations x 3/2 x u; second-order terms are below u^2 x 100.  A sharper count (4.5u relative on q after the normalisation, 3u
on the rotation's sum, u on R: 8.5u) lies inside it.  It is derived, not fitted: nothing here looks at what any code gives.
"""
import numpy as np

FP32_BOUND = 14 * 1.5 * 2.0 ** -24


def normal_f64(n, scale, R, scale_shift):
    """[...,3] float64: how a direction vector follows x' = R (S x) + shift - the inverse transpose of the linear part, R S^-1, and back
    to unit length; a zero vector stays zero.  Without scale_shift only the rotation (lengths kept)."""
    q = np.asarray(n, dtype=np.float64)
    if scale_shift:
        q = q / np.asarray(scale, dtype=np.float64)
        length = np.sqrt((q * q).sum(-1, keepdims=True))
        q = np.divide(q, length, out=q.copy(), where=length > 0)
    return q @ np.asarray(R, dtype=np.float64).T


def points_f64(attr, ref, attr_vectors, scale_shift):
    B, N = ref["perm"].shape
    A = attr.shape[2]
    out = np.zeros((B, A, N))
    for b in range(B):
        rows = attr[ref["m"][b], ref["perm"][b]].astype(np.float64)            # [N,A]
        for k in range(attr_vectors):
            rows[:, 3 * k:3 * k + 3] = normal_f64(rows[:, 3 * k:3 * k + 3], ref["scale"][b], ref["R"][b], scale_shift)
        out[b] = rows.T
    return out


def points_fp32(attr, ref, params, attr_vectors, scale_shift, rotate):
    """numpy float32 arithmetic rounds once per operation, never contracts, and divides and takes roots correctly rounded."""
    params = np.asarray(params, dtype=np.float32)
    B, N = ref["perm"].shape
    A = attr.shape[2]
    out = np.zeros((B, A, N), np.float32)
    for b in range(B):
        v = attr[ref["m"][b], ref["perm"][b]].astype(np.float32).T.copy()      # [A,N]; scalar channels: these bits
        for k in range(attr_vectors):
            q = v[3 * k:3 * k + 3].copy()
            if scale_shift:
                q = q / params[b, 0:3, None]
                l2 = ((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])
                length = np.sqrt(l2)
                assert length.dtype == np.float32
                pos = length > 0
                q[:, pos] = q[:, pos] / length[pos]
            if rotate in ("z", "so3"):
                R = params[b, 6:15].reshape(3, 3)
                q = np.stack([((R[r, 0] * q[0]) + (R[r, 1] * q[1])) + (R[r, 2] * q[2]) for r in range(3)])
            assert q.dtype == np.float32
            v[3 * k:3 * k + 3] = q
        out[b] = v
    return out
