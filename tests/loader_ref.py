"""Helper (not a test): a numpy restatement of one assembled batch, written from the derivation in svnet_amd/data.py's docstring -
not from the kernel, and sharing no code with the product (its own splitmix64, its own order, its own arithmetic).

    ref = batch(data, label, seg, seed=..., epoch=..., first=..., count=..., B=..., N=..., select=..., scale_shift=..., rotate=...,
                order=..., num_cat=...)
    ref["perm"] [B,N] pool point of every output slot     ref["y"] [B]   ref["seg"] [B,N]   ref["onehot"] [B,num_cat]
    ref["scale"], ref["shift"] [B,3] float32 (bit-exact)   ref["R"] [B,3,3] float64          ref["x"] [B,3,N] float64 (R in float64)
    x_fp32(data, ref, params) [B,3,N] float32: the coordinates evaluated in fp32, operation by operation, with a given `params`
    [B,16] (the device's own): what the kernel's x must equal bit for bit.
"""
import numpy as np

MASK = (1 << 64) - 1
SELECT = ("first_shuffled", "subset", "first_ordered")


def sm(x):
    """splitmix64 on Python ints."""
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sm_vec(x):
    """splitmix64 on a uint64 array (wrapping)."""
    x = np.asarray(x, dtype=np.uint64)
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def epoch_key(seed, epoch):
    return sm(sm(seed & MASK) ^ (epoch & MASK))


def cloud_key(seed, epoch, g):
    return sm(epoch_key(seed, epoch) ^ g)


def epoch_order(seed, epoch, M):
    order_key = sm(epoch_key(seed, epoch) ^ MASK)
    keys = [(((sm((order_key + i) & MASK)) >> 32) << 32) | i for i in range(M)]
    return np.array(sorted(range(M), key=lambda i: keys[i]), dtype=np.int64)


def point_keys(ck, S):
    p = np.arange(S, dtype=np.uint64)
    return ((sm_vec(np.uint64(ck) + p) >> np.uint64(16)) << np.uint64(16)) | p


def point_order(ck, P, N, select):
    """Pool point of every output slot, [N]."""
    if select == "first_ordered":
        return np.arange(N, dtype=np.int64)
    S = N if select == "first_shuffled" else P
    keys = point_keys(ck, S)
    assert len(np.unique(keys)) == S
    return np.argsort(keys, kind="stable")[:N].astype(np.int64)


def uniform(ck, j):
    """u_j as a float32 (exact: 24 bits)."""
    return np.float32((sm((ck + (1 << 32) + j) & MASK) >> 40) * 2.0 ** -24)


def scale_shift_of(ck):
    f = np.float32
    lo, span, slo, sspan = f(2.0 / 3.0), f(3.0 / 2.0 - 2.0 / 3.0), f(-0.2), f(0.4)
    scale = np.array([lo + span * uniform(ck, c) for c in range(3)], dtype=np.float32)
    shift = np.array([slo + sspan * uniform(ck, 3 + c) for c in range(3)], dtype=np.float32)
    return scale, shift


def rotation_of(ck, rotate):
    """float64 3x3 (the uniforms themselves are exact)."""
    if rotate == "z":
        t = 2.0 * np.pi * float(uniform(ck, 6))
        c, s = np.cos(t), np.sin(t)
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if rotate == "so3":
        u1, t2, t3 = float(uniform(ck, 6)), 2.0 * np.pi * float(uniform(ck, 7)), 2.0 * np.pi * float(uniform(ck, 8))
        a, b = np.sqrt(1.0 - u1), np.sqrt(u1)
        w, i, j, k = b * np.cos(t3), a * np.sin(t2), a * np.cos(t2), b * np.sin(t3)
        return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                         [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                         [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])
    return np.eye(3)


def batch(data, label, seg=None, *, seed, epoch, first, count, B, N, select, scale_shift, rotate, order=None, num_cat=None):
    M, P, _ = data.shape
    order = np.arange(M, dtype=np.int64) if order is None else order
    out = {"perm": np.zeros((B, N), np.int64), "y": np.zeros(B, np.int64), "scale": np.ones((B, 3), np.float32),
           "shift": np.zeros((B, 3), np.float32), "R": np.zeros((B, 3, 3)), "x": np.zeros((B, 3, N)), "m": np.zeros(B, np.int64)}
    if seg is not None:
        out["seg"] = np.zeros((B, N), np.int64)
    if num_cat is not None:
        out["onehot"] = np.zeros((B, num_cat), np.float32)
    for b in range(B):
        g = first + (b if b < count else 0)                 # slots past the valid count repeat slot 0
        m = int(order[g])
        ck = cloud_key(seed, epoch, g)
        perm = point_order(ck, P, N, select)
        pts = data[m, perm].astype(np.float64)              # [N,3]
        if scale_shift:
            out["scale"][b], out["shift"][b] = scale_shift_of(ck)
            pts = (data[m, perm] * out["scale"][b] + out["shift"][b]).astype(np.float64)     # fp32: two single-rounded operations
        R = rotation_of(ck, rotate)
        out["R"][b] = R
        out["x"][b] = R @ pts.T
        out["perm"][b], out["y"][b], out["m"][b] = perm, label[m], m
        if seg is not None:
            out["seg"][b] = seg[m, perm]
        if num_cat is not None and 0 <= label[m] < num_cat:
            out["onehot"][b, label[m]] = 1.0
    return out


def x_fp32(data, ref, params, scale_shift, rotate):
    """[B,3,N] float32 from the reference's point order and the given params [B,16] (3 scales, 3 shifts, 9 rotation entries, pad),
    in the docstring's operation order; numpy float32 arithmetic rounds once per operation and never contracts."""
    params = np.asarray(params, dtype=np.float32)
    B, N = ref["perm"].shape
    out = np.zeros((B, 3, N), np.float32)
    for b in range(B):
        v = data[ref["m"][b], ref["perm"][b]].astype(np.float32).T.copy()       # [3,N]
        if scale_shift:
            v = (v * params[b, 0:3, None]) + params[b, 3:6, None]
        if rotate in ("z", "so3"):
            R = params[b, 6:15].reshape(3, 3)
            v = np.stack([((R[r, 0] * v[0]) + (R[r, 1] * v[1])) + (R[r, 2] * v[2]) for r in range(3)])
        out[b] = v
    return out
