"""A plain numpy restatement of the binarized dense layer (sv_layers.py:35-51 with bw and ba; svnet_amd/csrc/binlinear.hip,
binlinear_mfma.hip), for tests/binlinear_cases.py:

    t = float32(x) + float32(beta)          one float32 add
    x_b = sign(t), sign(0) = 0              ternary
    count = x_b . sign(W)^T                 an integer, |count| <= K
    y = count * scale (+ bias)

and of what goes with it: the three row-sliced planes the forward saves, the weight planes and values of svnet_binweight_prepare_f32,
the column sums the matrix-core kernel leaves for the BatchNorm, and the gradient epilogue svnet_binweight_grad_f32.  The permuted int8
weight packing of the matrix-core kernel is NOT restated: it is internal to that kernel, and the forward cases test it end to end.
Nothing here imports the package under test."""
import numpy as np

STE = np.float32(1.2)          # the straight-through window: |t| <= float32(1.2)


def binarize(x, beta):
    """t [M,K] float32 and the sign / non-zero / STE booleans of the binarized input."""
    assert x.dtype == np.float32 and beta.dtype == np.float32
    t = x + beta[None, :]
    assert t.dtype == np.float32
    return t, t > 0, t != 0, np.abs(t) <= STE


def ternary(pos, nz):
    return np.where(nz, np.where(pos, 1, -1), 0).astype(np.int8)


def weight_sign(W):
    return ((W > 0).astype(np.int8) - (W < 0).astype(np.int8))


def counts(xb, wb):
    """count [M,O] int64 = xb . wb^T of two ternary operands.  Formed as a float64 product (|count| <= K < 2^53: every partial sum is an
    exactly represented integer whatever the order) and converted."""
    c = xb.astype(np.float64) @ wb.astype(np.float64).T
    out = c.astype(np.int64)
    assert np.array_equal(out.astype(np.float64), c)
    return out


def row_sliced(bits):
    """bits [M,K] bool -> uint64 [ceil(M/64), K]: word [(m >> 6) * K + k] holds row m's bit at position m & 63; rows past M are 0."""
    M, K = bits.shape
    MB = (M + 63) // 64
    b = np.zeros((MB * 64, K), np.uint8)
    b[:M] = bits
    b = np.ascontiguousarray(b.reshape(MB, 64, K).transpose(0, 2, 1))              # [MB, K, 64]
    return np.packbits(b, axis=-1, bitorder="little").view(np.uint64).reshape(MB, K)


def row_words(bits):
    """bits [O,K] bool -> uint64 [O, ceil(K/64)]: word [o, k >> 6] holds column k's bit at position k & 63 (the weight planes)."""
    O, K = bits.shape
    KW = (K + 63) // 64
    b = np.zeros((O, KW * 64), np.uint8)
    b[:, :K] = bits
    return np.packbits(b.reshape(O, KW, 64), axis=-1, bitorder="little").view(np.uint64).reshape(O, KW)


def weight_prepare(W, scale=None):
    """(w_sign, w_nz, w_b, w_eff) of svnet_binweight_prepare_f32; w_eff is None without scale."""
    wb = weight_sign(W).astype(np.float32)
    w_eff = None if scale is None else wb * scale.astype(np.float32)[:, None]      # (+-scale or 0: exact)
    return row_words(W > 0), row_words(W != 0), wb, w_eff


def forward(x, beta, W, scale, bias=None, cloud_n=None, rows_per_cloud=0):
    """A dict of the layer's exact results: count [M,O] int64 (cloud_n [M / rows_per_cloud, O], integer valued, added per cloud),
    y [M,O] float64 = count * scale + bias without rounding error beyond float64's, mag = |count * scale|, and the three planes."""
    t, pos, nz, ste = binarize(x, beta)
    cnt = counts(ternary(pos, nz), weight_sign(W))
    if cloud_n is not None:
        add = cloud_n.astype(np.int64)
        assert np.array_equal(add.astype(cloud_n.dtype), cloud_n) and x.shape[0] % rows_per_cloud == 0
        cnt = cnt + np.repeat(add, rows_per_cloud, axis=0)
    prod = cnt.astype(np.float64) * scale.astype(np.float64)[None, :]
    y = prod if bias is None else prod + bias.astype(np.float64)[None, :]
    return dict(t=t, count=cnt, y=y, mag=np.abs(prod), x_sign=row_sliced(pos), x_nz=row_sliced(nz), x_ste=row_sliced(ste))


def col_sums(count, scale, bias=None):
    """(sums [2 O] float64 = [sum_m y | sum_m y^2], brackets [2 O]) from the exact integer S1 = sum count, S2 = sum count^2:
    sum y = s S1 + M b, sum y^2 = s^2 S2 + 2 s b S1 + M b^2.  The bracket is the sum of the magnitudes of the terms:
    sum_m (|s c_m| + |b|) and sum_m (s^2 c_m^2 + 2 |s b c_m| + b^2)."""
    M = count.shape[0]
    s = scale.astype(np.float64)
    b = np.zeros_like(s) if bias is None else bias.astype(np.float64)
    S1, S2, A1 = count.sum(axis=0), (count * count).sum(axis=0), np.abs(count).sum(axis=0)
    s1, s2, a1 = S1.astype(np.float64), S2.astype(np.float64), A1.astype(np.float64)
    sums = np.concatenate([s * s1 + M * b, s * s * s2 + 2.0 * s * b * s1 + M * b * b])
    mags = np.concatenate([np.abs(s) * a1 + M * np.abs(b), s * s * s2 + 2.0 * np.abs(s * b) * a1 + M * b * b])
    return sums, mags


def weight_grad(GX, W, scale):
    """float64 (dW [O,K], dscale [O]) of the epilogue, and the magnitudes of dscale's terms summed: dW = [|W| <= 1.2] scale GX,
    dscale = sum_k sign(W) GX.  GX: float64 [O,K] (a sliced input summed by the caller)."""
    inside = np.abs(W) <= STE
    dW = np.where(inside, scale.astype(np.float64)[:, None] * GX, 0.0)
    terms = weight_sign(W).astype(np.float64) * GX
    return dW, terms.sum(axis=1), np.abs(terms).sum(axis=1)
