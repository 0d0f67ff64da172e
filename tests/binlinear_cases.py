"""The case list of the binarized dense layer's kernels, stated once: tests/test_host_binlinear_cases.py (CPU: the tier queries, the
restatement, the comparators' teeth) and tests/test_hip_binlinear_tiers.py (GPU: every case against tests/binlinear_ref.py) iterate the
same tables.

  POPCOUNT   svnet_binlinear_fwd_f32 (binlinear_fwd_kernel<KWM, PPM>): a case names, per column chunk, KW and KWM, then PPM, the launch
             form, og_shift, o_blocks, the number of launches and the grid's row-tile count it is MEANT to reach.
  I8         svnet_binlinear_i8_fwd_f32 / svnet_binlinear_i8_cloud_fwd_f32 (binlinear_i8_fwd_kernel<NTW>): NTW, the grid, the number of
             128-column chunks, LDS bytes.
  PREPARE    svnet_binweight_prepare_f32.          GRAD   svnet_binweight_grad_f32.
The expectations are written out by hand from the dispatch rules (KINFO, FORMS, the literal arguments of i8()), never computed from
the code under test: a case that silently falls through to another tier fails the query assertion before anything runs.

Every case calls the C interface directly.  From Python (_ops.BinLinear) M >= 1024 and O >= 64 goes to the matrix-core kernel while
config.BINLINEAR_MFMA is on, so PPM = 2 and the PPM = 1 loop over o_base with several launches (both need more than 4096 pairs of a row
tile and a 256-channel group, i.e. O > 256 and far more than 1024 rows) are reachable from Python only with BINLINEAR_MFMA = False; the
matrix-core kernel below 1024 rows or 64 channels, ldx > K, a forward without bias through the matrix cores without column sums, and
svnet_binweight_grad_f32's combinations of accumulate / gx_sliced / sum_buf are reachable through the C interface alone.

Every forward case runs with two value kinds:
  exact  scale a power of two in {0.25, 0.5, 1, 2}, bias an integer multiple of 1/8: count * scale + bias is exact in float32 whether or
         not the compiler contracts it to an fma, and y must equal the reference BIT FOR BIT (-0 counted as +0).
  real   scale in [0.5, 1.5], bias standard normal: |y - ref64| <= 2^-24 (|count scale| + |ref64|) per element - the two roundings of
         fl(fl(count scale) + bias) (each at most 2^-24 / (1 + 2^-24) of its exact argument), which also covers the single rounding of
         the fma form.  Derived, not measured.
Planes and svnet_binweight_prepare_f32's outputs are bit-equal in both kinds.

x, W and beta are float32 standard normals with planted exact zeros, -0.0, entries with x == -beta (t == 0) and entries with
|t| == float32(1.2) and |t| == nextafter(float32(1.2), 2) in both signs; no NaN, Inf or denormals.  Every output has a guard: y two
trailing sentinel rows, each plane one extra 64-row block; with ldx > K the pad columns of x hold a large finite value."""
import zlib

import numpy as np

from svnet_amd import _lib
from tests import binlinear_ref as R

D = _lib.DEFINES
TILE_SPLIT, GROUPS, LOOP = D["SVNET_BINLINEAR_TILE_SPLIT"], D["SVNET_BINLINEAR_GROUPS"], D["SVNET_BINLINEAR_LOOP"]
FORM = {TILE_SPLIT: "TILE_SPLIT", GROUPS: "GROUPS", LOOP: "LOOP"}
E_ARG, E_UNSUPPORTED = D["SVNET_E_ARG"], D["SVNET_E_UNSUPPORTED"]
RED_SLICES = D["SVNET_RED_SLICES"]

EPS24, EPS52 = 2.0 ** -24, 2.0 ** -52
KINDS = ("exact", "real")
Y_SENTINEL = -777.0
PLANE_SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD_VALUE = 1.0e30
Y_GUARD_ROWS = 2
F12 = np.float32(1.2)
F12_UP = np.nextafter(np.float32(1.2), np.float32(2))


def sliced_len(L):
    return (RED_SLICES + 1) * L + 2         # SVNET_SLICED_LEN


# ----------------------------------------------------------------------------- the popcount kernel
# K -> (words per chunk, [(KW, KWM) per chunk]): ceil(K / 64) words; more than 34 are cut into ceil(words / 34) chunks of equal whole
# words, the last chunk takes what is left; KWM is the smallest of 2, 4, 8, 16, 34 that holds KW
KINFO = {
    1: (1, [(1, 2)]), 3: (1, [(1, 2)]), 64: (1, [(1, 2)]), 65: (2, [(2, 2)]), 70: (2, [(2, 2)]), 128: (2, [(2, 2)]),
    129: (3, [(3, 4)]), 130: (3, [(3, 4)]), 256: (4, [(4, 4)]), 257: (5, [(5, 8)]), 300: (5, [(5, 8)]), 512: (8, [(8, 8)]),
    513: (9, [(9, 16)]), 1024: (16, [(16, 16)]), 1025: (17, [(17, 34)]), 2176: (34, [(34, 34)]),
    2177: (18, [(18, 34), (17, 34)]),               # 35 words
    2240: (18, [(18, 34), (17, 34)]),               # 35 words, the last one full
    4353: (23, [(23, 34), (23, 34), (23, 34)]),     # 69 words
}
# (M, O) -> (form, og_shift, o_blocks, launches, row tiles of the grid) at PPM = 1.  tiles = ceil(M / 64).
#   TILE_SPLIT  tiles <= 8 and O > 32: og_shift 5, ceil(O / 32) workgroups per tile
#   GROUPS      otherwise O > 256 and tiles * ceil(O / 256) <= 4096: og_shift 8, ceil(O / 256) workgroups per tile
#   LOOP        otherwise: og_shift = the smallest of 5 .. 8 with 2^og_shift >= O (8 beyond), ceil(O / 256) launches, min(tiles, 2048)
FORMS = {
    (1, 33): (TILE_SPLIT, 5, 2, 1, 1), (1, 64): (TILE_SPLIT, 5, 2, 1, 1), (1, 65): (TILE_SPLIT, 5, 3, 1, 1),
    (63, 33): (TILE_SPLIT, 5, 2, 1, 1), (63, 64): (TILE_SPLIT, 5, 2, 1, 1), (63, 65): (TILE_SPLIT, 5, 3, 1, 1),
    (64, 33): (TILE_SPLIT, 5, 2, 1, 1), (64, 64): (TILE_SPLIT, 5, 2, 1, 1), (64, 65): (TILE_SPLIT, 5, 3, 1, 1),
    (65, 33): (TILE_SPLIT, 5, 2, 1, 2), (65, 64): (TILE_SPLIT, 5, 2, 1, 2), (65, 65): (TILE_SPLIT, 5, 3, 1, 2),
    (512, 33): (TILE_SPLIT, 5, 2, 1, 8), (512, 64): (TILE_SPLIT, 5, 2, 1, 8), (512, 65): (TILE_SPLIT, 5, 3, 1, 8),
    (513, 257): (GROUPS, 8, 2, 1, 9), (513, 512): (GROUPS, 8, 2, 1, 9), (513, 513): (GROUPS, 8, 3, 1, 9),
    (1, 1): (LOOP, 5, 1, 1, 1), (5, 5): (LOOP, 5, 1, 1, 1), (70, 32): (LOOP, 5, 1, 1, 2), (512, 32): (LOOP, 5, 1, 1, 8),
    (513, 1): (LOOP, 5, 1, 1, 9), (513, 32): (LOOP, 5, 1, 1, 9), (513, 33): (LOOP, 6, 1, 1, 9), (513, 64): (LOOP, 6, 1, 1, 9),
    (513, 65): (LOOP, 7, 1, 1, 9), (513, 128): (LOOP, 7, 1, 1, 9), (513, 129): (LOOP, 8, 1, 1, 9), (513, 256): (LOOP, 8, 1, 1, 9),
}
BIG_M = 131073                                       # 2049 row tiles: one more than the grid's cap

POPCOUNT = []


def pop(name, M, K, O, planes=1, bias=1, ldx_pad=0, ppm=1, form=None, device=0):
    assert all(c["name"] != name for c in POPCOUNT), name
    wpc, chunks = KINFO[K]
    POPCOUNT.append(dict(name=name, M=M, K=K, O=O, planes=planes, bias=bias, ldx_pad=ldx_pad, ppm=ppm, wpc=wpc, chunks=chunks,
                         form=form if form is not None else FORMS[(M, O)], device=device))


# ---- every K edge in each of the three launch forms (the WIDE template and the chunked K crossed with all of them)
_TS = [(1, 33), (63, 64), (64, 65), (65, 33), (512, 64)]
_GR = [(513, 257), (513, 512), (513, 513)]
_LO = [(513, 32), (513, 33), (513, 64), (513, 65), (513, 128), (513, 129), (513, 256)]
for _i, _k in enumerate((1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2176, 2177, 2240, 4353)):
    pop("k%d_split" % _k, *_TS[_i % 5][:1], _k, _TS[_i % 5][1])
    pop("k%d_groups" % _k, 513, _k, _GR[_i % 3][1])
    pop("k%d_loop" % _k, 513, _k, _LO[_i % 7][1])
# ---- the tile-split form: every M with every O
for _m in (1, 63, 64, 65, 512):
    for _o in (33, 64, 65):
        pop("split_%dx%d" % (_m, _o), _m, 70, _o, planes=(_m + _o) & 1)
# ---- the loop over o_base: O <= 32 at any M, and more than 8 tiles with every og_shift
for _m, _o in ((1, 1), (5, 5), (70, 32), (512, 32), (513, 1)):
    pop("loop_%dx%d" % (_m, _o), _m, 129, _o)
for _o in (32, 33, 64, 65, 128, 129, 256):
    pop("loop_og_%d" % _o, 513, 300, _o, planes=_o & 1)
# ---- WIDE (KW > 16): both loop branches (og_shift < 8: a row at a time; og_shift = 8: 64 row counters per thread)
for _k in (1025, 2176):
    pop("wide%d_loop_og5" % _k, 70, _k, 32)
    pop("wide%d_loop_og7" % _k, 513, _k, 128, planes=0)
    pop("wide%d_loop_og8" % _k, 513, _k, 129)
    pop("wide%d_loop_og8_256" % _k, 513, _k, 256, planes=0)
# ---- chunked K with all three forms, with and without planes (the sweep above saves them)
for _k in (2177, 2240, 4353):
    pop("chunk%d_split_noplanes" % _k, 65, _k, 65, planes=0)
    pop("chunk%d_groups_noplanes" % _k, 513, _k, 257, planes=0)
    pop("chunk%d_loop_og6_noplanes" % _k, 513, _k, 33, planes=0)
    pop("chunk%d_loop_og8" % _k, 513, _k, 129)
    pop("chunk%d_loop_og8_noplanes" % _k, 513, _k, 256, planes=0)
# ---- ldx = K + 5, once per KWM (and once per chunked K: the chunks' pointers are offset by col0 inside a padded row)
for _k in (70, 130, 300, 513, 1025, 2177):
    pop("ldx_k%d" % _k, 65, _k, 33, ldx_pad=5)
pop("ldx_k4353_groups", 513, 4353, 257, ldx_pad=5)
# ---- O = 1 and no bias
pop("o1_m70", 70, 70, 1, form=(LOOP, 5, 1, 1, 2))
pop("nobias_split", 65, 129, 65, bias=0)
pop("nobias_groups", 513, 257, 512, bias=0)
pop("nobias_loop_wide", 513, 1025, 65, bias=0)
pop("nobias_chunked", 65, 2177, 33, bias=0, planes=0)
# ---- beyond 131072 rows (2049 tiles x 2 channel groups > 4096 pairs): inputs and reference built on the device
pop("big_ppm2_kwm2", BIG_M, 3, 257, planes=0, ppm=2, form=(LOOP, 8, 1, 1, 2048), device=1)
pop("big_ppm2_kwm4", BIG_M, 130, 257, planes=0, ppm=2, form=(LOOP, 8, 1, 1, 2048), device=1)
pop("big_ppm2_kwm8", BIG_M, 300, 257, planes=0, ppm=2, form=(LOOP, 8, 1, 1, 2048), device=1)
pop("big_ppm1_two_launches", BIG_M, 513, 257, planes=0, form=(LOOP, 8, 1, 2, 2048), device=1)
pop("big_second_tile_pass", BIG_M, 3, 5, planes=0, form=(LOOP, 5, 1, 1, 2048), device=1)

POPCOUNT_HOST = [c for c in POPCOUNT if not c["device"]]
POPCOUNT_DEVICE = [c for c in POPCOUNT if c["device"]]


def expected_plan(c, chunk):
    """The fields of svnet_binlinear_plan a case expects for one chunk, from the hand-written tables."""
    form, og, ob, launches, grid = c["form"]
    kw, kwm = c["chunks"][chunk]
    n = len(c["chunks"])
    kc = c["wpc"] * 64 if chunk + 1 < n else c["K"] - chunk * c["wpc"] * 64
    return dict(nchunk=n, wpc=c["wpc"], chunk=chunk, col0=chunk * c["wpc"] * 64, kc=kc, kw=kw, kwm=kwm, ppm=c["ppm"], form=form,
                og_shift=og, o_blocks=ob, launches=launches, grid_tiles=grid, ymode=(1 if chunk else 0) | (2 if chunk + 1 < n else 0),
                lds_bytes=3 * 64 * kw * 8)


def plan_of(c, chunk):
    p = _lib.STRUCTS["svnet_binlinear_plan"]()
    rc = _lib.lib().svnet_binlinear_tier(c["M"], c["K"], c["O"], chunk, p)
    return rc, {f: getattr(p, f) for f, _ in p._fields_}


# ----------------------------------------------------------------------------- the matrix-core kernel
I8_LDS = {1: 43008, 2: 61440, 4: 98304}              # 128 x 144 (A) + 128 NTW x 144 (B) + 3 x 128 x 2 x 8 (plane words)
I8 = []


def i8(name, M, K, O, ntw, gx, gy, nch, planes=0, sums=0, cloud=0, bias=1, ldx_pad=0):
    """cloud: rows_per_cloud (0 = svnet_binlinear_i8_fwd_f32)."""
    assert all(c["name"] != name for c in I8), name
    I8.append(dict(name=name, M=M, K=K, O=O, ntw=ntw, grid_x=gx, grid_y=gy, nchunks=nch, planes=planes, sums=sums, cloud=cloud, bias=bias,
                   ldx_pad=ldx_pad))


# a pairwise table: every M, K and O of the lists below, every NTW x {planes, sums, cloud} combination
#   M 1 8 63 64 65 127 128 129 200 257 (600: two clouds of 300)    K 1 31 32 33 127 128 129 255 256 257 300
#   O 1 31 32 33 128 | 129 256 | 257 512 513 1025                   rows_per_cloud 1 7 128 300 M
i8("n1_000", 1, 1, 1, 1, 1, 1, 1, bias=0)
i8("n1_p00", 8, 31, 31, 1, 1, 1, 1, planes=1)
i8("n1_0s0", 63, 32, 32, 1, 1, 1, 1, sums=1, ldx_pad=5)
i8("n1_ps0", 64, 33, 33, 1, 1, 1, 1, planes=1, sums=1, bias=0)
i8("n1_00c1", 65, 127, 128, 1, 1, 1, 1, cloud=1)
i8("n1_p0c7", 63, 128, 1, 1, 1, 1, 1, planes=1, cloud=7, ldx_pad=5)
i8("n1_0sc128", 128, 129, 31, 1, 1, 1, 2, sums=1, cloud=128, bias=0)
i8("n1_psc300", 600, 255, 33, 1, 5, 1, 2, planes=1, sums=1, cloud=300)
i8("n2_000", 127, 256, 129, 2, 1, 1, 2, ldx_pad=5)
i8("n2_p00", 128, 257, 256, 2, 1, 1, 3, planes=1, bias=0)
i8("n2_0s0", 129, 300, 129, 2, 2, 1, 3, sums=1)
i8("n2_ps0", 200, 1, 256, 2, 2, 1, 1, planes=1, sums=1, ldx_pad=5)
i8("n2_00cM", 257, 31, 129, 2, 3, 1, 1, cloud=257, bias=0)
i8("n2_p0c1", 1, 32, 256, 2, 1, 1, 1, planes=1, cloud=1)
i8("n2_0scM", 8, 33, 129, 2, 1, 1, 1, sums=1, cloud=8, ldx_pad=5)
i8("n2_psc7", 63, 127, 256, 2, 1, 1, 1, planes=1, sums=1, cloud=7, bias=0)
i8("n4_000", 64, 128, 257, 4, 1, 1, 1)
i8("n4_p00", 65, 129, 512, 4, 1, 1, 2, planes=1, ldx_pad=5)
i8("n4_0s0_y2", 127, 255, 513, 4, 1, 2, 2, sums=1, bias=0)
i8("n4_ps0_y3", 128, 256, 1025, 4, 1, 3, 2, planes=1, sums=1)
i8("n4_00c1", 129, 257, 257, 4, 2, 1, 3, cloud=1, ldx_pad=5)
i8("n4_p0cM", 200, 300, 512, 4, 2, 1, 3, planes=1, cloud=200, bias=0)
i8("n4_0sc1_y2", 257, 1, 513, 4, 3, 2, 1, sums=1, cloud=1)
i8("n4_psc300_y3", 600, 31, 1025, 4, 5, 3, 1, planes=1, sums=1, cloud=300, ldx_pad=5)
i8("n4_psc128", 128, 300, 512, 4, 1, 1, 3, planes=1, sums=1, cloud=128, ldx_pad=5)
i8("n4_ps0_y2_m257", 257, 129, 513, 4, 3, 2, 2, planes=1, sums=1)
i8("n1_ps0_m129", 129, 256, 128, 1, 2, 1, 2, planes=1, sums=1)
i8("n1_psc128_m256", 256, 33, 32, 1, 2, 1, 1, planes=1, sums=1, cloud=128)             # one cloud per workgroup
i8("n2_psc7_m63x3", 189, 257, 129, 2, 2, 1, 3, planes=1, sums=1, cloud=7)             # a workgroup spans 18 clouds and a part of one


def expected_i8_plan(c):
    return dict(ntw=c["ntw"], grid_x=c["grid_x"], grid_y=c["grid_y"], nchunks=c["nchunks"], kp=128 * c["nchunks"], lds_bytes=I8_LDS[c["ntw"]])


def i8_plan_of(c):
    p = _lib.STRUCTS["svnet_binlinear_i8_plan"]()
    rc = _lib.lib().svnet_binlinear_i8_tier(c["M"], c["K"], c["O"], c["sums"], p)
    return rc, {f: getattr(p, f) for f, _ in p._fields_}


# ----------------------------------------------------------------------------- weight preparation and the gradient epilogue
PREPARE = [dict(name="prep_%dx%d_%s" % (o, k, mode), O=o, K=k, mode=mode)
           for o, k in ((1, 1), (3, 63), (5, 64), (7, 65), (40, 130)) for mode in ("all", "noscale", "planes")]
# mode: "all" scale, w_b, w_eff and planes; "noscale" w_b and planes, scale and w_eff NULL; "planes" the two planes alone

GRAD = []
for _o, _k in ((1, 1), (3, 63), (5, 65), (40, 130), (5000, 3)):                  # (5000 rows: more than the grid's 4096 waves)
    for _acc, _eval, _sl, _sum in ((0, 0, 0, 0), (1, 0, 0, 1), (0, 0, 1, 65), (1, 0, 1, 0), (0, 1, 0, 65), (1, 1, 1, 1)):
        GRAD.append(dict(name="grad_%dx%d_a%d_e%d_s%d_b%d" % (_o, _k, _acc, _eval, _sl, _sum), O=_o, K=_k, accumulate=_acc, eval=_eval,
                         gx_sliced=_sl, sum_len=_sum))


def by_name(table, name):
    return next(c for c in table if c["name"] == name)


# ----------------------------------------------------------------------------- values
class Data:
    pass


def _rng(c, kind):
    return np.random.default_rng(zlib.crc32(("%s/%s" % (c["name"], kind)).encode()))


def _pick(rng, n, frac, least=1):
    """Flat indices of about frac * n elements (at least `least` when n allows)."""
    m = min(n, max(least, int(n * frac)))
    return rng.choice(n, size=m, replace=False)


def scale_bias(rng, O, kind, bias=True):
    if kind == "exact":
        sc = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), size=O)
        bs = (rng.integers(-32, 33, size=O) / 8.0).astype(np.float32)
    else:
        sc = rng.uniform(0.5, 1.5, size=O).astype(np.float32)
        bs = rng.standard_normal(size=O, dtype=np.float32)
    return sc, (bs if bias else None)


def plant_weights(rng, W):
    """Exact zeros, -0.0 and the |W| = 1.2 boundary (both sides, both signs) in a weight matrix."""
    f = W.reshape(-1)
    f[_pick(rng, f.size, 0.06)] = 0.0
    f[_pick(rng, f.size, 0.02, 0)] = -0.0
    for v in (F12, -F12, F12_UP, -F12_UP):
        f[_pick(rng, f.size, 0.02, 1 if f.size >= 8 else 0)] = v
    return W


def build_forward(c, kind):
    """x (storage [M, ldx] with the pad columns at PAD_VALUE, and the [M, K] view), beta, W, scale, bias, cloud_n of a forward case."""
    M, K, O = c["M"], c["K"], c["O"]
    rng = _rng(c, kind)
    d = Data()
    d.kind, d.ldx = kind, K + c["ldx_pad"]
    d.x_store = np.full((M, d.ldx), PAD_VALUE, np.float32)
    x = rng.standard_normal(size=(M, K), dtype=np.float32)
    beta = rng.standard_normal(size=K, dtype=np.float32)
    beta[_pick(rng, K, 0.2)] = 0.0
    if K >= 4:
        beta[_pick(rng, K, 0.05)] = -0.0
    xf = x.reshape(-1)
    xf[_pick(rng, xf.size, 0.05)] = 0.0
    xf[_pick(rng, xf.size, 0.02, 0)] = -0.0
    col = np.arange(xf.size) % K
    at = _pick(rng, xf.size, 0.03)
    xf[at] = -beta[col[at]]                                                        # t == 0 exactly (x + (-x) = 0)
    d.hits = {}
    for v in (F12, -F12, F12_UP, -F12_UP):                                         # |t| on and one ulp above the STE threshold
        at = _pick(rng, xf.size, 0.03)
        cand = (v - beta[col[at]]).astype(np.float32)
        ok = (cand + beta[col[at]]) == v                                           # (always where beta is 0; elsewhere when the two roundings cancel)
        xf[at[ok]] = cand[ok]
        d.hits[float(v)] = int(ok.sum())
    d.x_store[:, :K] = x
    d.x = d.x_store[:, :K]
    d.beta = beta
    d.W = plant_weights(rng, rng.standard_normal(size=(O, K), dtype=np.float32))
    d.scale, d.bias = scale_bias(rng, O, kind, c["bias"])
    d.cloud_n = None
    if c.get("cloud"):
        d.cloud_n = rng.integers(-1600, 1601, size=(M // c["cloud"], O)).astype(np.float32)
    assert np.isfinite(d.x_store).all() and np.isfinite(d.W).all()
    return d


def reference_forward(c, d, ste=None):
    r = R.forward(d.x, d.beta, d.W, d.scale, d.bias, d.cloud_n, c.get("cloud", 0))
    if ste is not None:                                                            # (the teeth checks: a window with another threshold)
        r["x_ste"] = R.row_sliced(np.abs(r["t"]) <= ste)
    return r


def y_storage(c):
    return np.full((c["M"] + Y_GUARD_ROWS, c["O"]), Y_SENTINEL, np.float32)


def plane_storage(c):
    return np.full(((c["M"] + 63) // 64 + 1, c["K"]), PLANE_SENTINEL, np.uint64)


def y_failures(c, kind, r, y_store):
    """Why y (the whole storage, guard rows included) is not the reference; [] when it is."""
    out = []
    M = c["M"]
    y = np.asarray(y_store[:M], dtype=np.float64)
    if not np.all(y_store[M:] == np.float32(Y_SENTINEL)):
        out.append("%s [%s]: rows past M were written" % (c["name"], kind))
    if kind == "exact":
        bad = np.argwhere(y != r["y"])                                             # (value comparison: -0 == +0)
        if bad.size:
            i, j = bad[0]
            out.append("%s [exact]: %d of %d elements differ, first y(%d, %d) = %r, expected %r (count %d)"
                       % (c["name"], len(bad), y.size, i, j, y_store[i, j], r["y"][i, j], r["count"][i, j]))
        return out
    err, bound = np.abs(y - r["y"]), EPS24 * (r["mag"] + np.abs(r["y"]))
    bad = np.argwhere(~(err <= bound))
    if bad.size:
        i, j = bad[0]
        out.append("%s [real]: %d of %d elements out of bound, first y(%d, %d) = %r, expected %r, error %.3g, bound %.3g"
                   % (c["name"], len(bad), y.size, i, j, y_store[i, j], r["y"][i, j], err[i, j], bound[i, j]))
    return out


def plane_failures(c, r, planes):
    """planes: {"x_sign" | "x_nz" | "x_ste": uint64 storage [ceil(M/64) + 1, K]}."""
    out = []
    for name, got in planes.items():
        got = np.asarray(got).view(np.uint64)
        if not np.all(got[-1] == PLANE_SENTINEL):
            out.append("%s: the block past %s was written" % (c["name"], name))
        bad = np.argwhere(got[:-1] != r[name])
        if bad.size:
            b, k = bad[0]
            out.append("%s: %d words of %s differ, first block %d column %d: %#018x, expected %#018x"
                       % (c["name"], len(bad), name, b, k, int(got[b, k]), int(r[name][b, k])))
    return out


def exact_kind_is_exact(r):
    """The exact kind's claim: every y is a float32, so no rounding (and no fma) can show."""
    return np.array_equal(r["y"].astype(np.float32).astype(np.float64), r["y"])


def colsum_failures(c, r, d, got):
    """got: the 2 O totals of the sliced accumulator.  |got - ref| <= n 2^-52 sum|terms|, n = ceil(M / 128) partials + RED_SLICES slice
    additions: a workgroup forms its partial s S1 + R b (s^2 S2 + 2 s b S1 + R b^2) from exact integers in at most 7 double roundings, each
    at most 2^-53 of the partial's bracket; every one of the n additions rounds by at most 2^-53 of the whole bracket; 7 + n <= 2 n."""
    ref, mag = R.col_sums(r["count"], d.scale, d.bias)
    n = (c["M"] + 127) // 128 + RED_SLICES
    err, bound = np.abs(np.asarray(got, dtype=np.float64) - ref), n * EPS52 * mag
    bad = np.flatnonzero(~(err <= bound))
    if bad.size:
        j = int(bad[0])
        return ["%s: %d column sums out of bound, first [%d] = %r, expected %r, error %.3g, bound %.3g"
                % (c["name"], bad.size, j, got[j], ref[j], err[j], bound[j])]
    return []


# ---- the gradient epilogue
def build_grad(c, kind):
    O, K = c["O"], c["K"]
    L = O * K
    rng = _rng(c, kind)
    d = Data()
    d.kind = kind
    d.W = plant_weights(rng, rng.standard_normal(size=(O, K), dtype=np.float32))
    if kind == "exact":
        d.scale = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), size=O)
        vals = lambda shape: rng.integers(-8, 9, size=shape).astype(np.float32)
    else:
        d.scale = rng.uniform(0.5, 1.5, size=O).astype(np.float32)
        vals = lambda shape: rng.standard_normal(size=shape, dtype=np.float32)
    if c["gx_sliced"]:
        # the slices' float32 sum must itself be exact for the dW bound (which takes g as given) to apply: multiples of 2^-10 below 2^6
        # (small integers in the exact kind) - sixteen of them sum below 2^10 with 20 significant bits, in any order
        d.GX_store = np.zeros(sliced_len(L), np.float32)
        sl = rng.integers(-8, 9, size=(RED_SLICES, L)) if kind == "exact" else rng.integers(-(1 << 16) + 1, 1 << 16, size=(RED_SLICES, L)) / 1024.0
        d.GX_store[L:L + RED_SLICES * L] = sl.astype(np.float32).reshape(-1)
        d.GX_store[:L] = 99.0                                                      # (the totals are not read)
        d.GX = sl.astype(np.float64).sum(axis=0).reshape(O, K)
        d.gx_terms = RED_SLICES
    else:
        d.GX_store = vals((O, K))
        d.GX = d.GX_store.astype(np.float64)
        d.gx_terms = 1
    d.dW0, d.dscale0 = vals((O, K)), vals(O)
    d.sum_store = None
    if c["sum_len"]:
        n = c["sum_len"]
        d.sum_store = np.zeros(sliced_len(n), np.float32)
        d.sum_store[n:n + RED_SLICES * n] = vals(RED_SLICES * n)
        d.sum_store[:n] = 55.0
    return d


def grad_failures(c, d, dW, dscale, sum_buf):
    """dW (None in eval), dscale, sum_buf (the storage after the call, None without) against the float64 epilogue.
    exact: bit for bit.  real: dW to 2^-24 (|scale g| + |dW0| + |result|); dscale and the sum_buf totals to (n - 1) 2^-24 sum|term|, n the
    number of terms of each sum: K products (each of RED_SLICES slices when GX is sliced), one more with accumulate; RED_SLICES slices."""
    out = []
    O, K, acc = c["O"], c["K"], c["accumulate"]
    rW, rs, smag = R.weight_grad(d.GX, d.W, d.scale)
    wmag = np.abs(np.where(np.abs(d.W) <= R.STE, d.scale.astype(np.float64)[:, None] * d.GX, 0.0))
    n = K * d.gx_terms
    if acc:
        rW, wmag = rW + d.dW0, wmag + np.abs(d.dW0)
        rs, smag, n = rs + d.dscale0, smag + np.abs(d.dscale0), n + 1
    checks = [("dscale", dscale, rs, (n - 1) * EPS24 * smag)]
    if dW is not None:
        checks.append(("dW", dW, rW, EPS24 * (wmag + np.abs(rW))))
    if sum_buf is not None:
        m = c["sum_len"]
        sl = d.sum_store[m:m + RED_SLICES * m].astype(np.float64).reshape(RED_SLICES, m)
        checks.append(("sum_buf", sum_buf[:m], sl.sum(axis=0), (RED_SLICES - 1) * EPS24 * np.abs(sl).sum(axis=0)))
        if not np.array_equal(sum_buf[m:], d.sum_store[m:]):
            out.append("%s: sum_buf's slices were changed" % c["name"])
    for what, got, ref, bound in checks:
        got = np.asarray(got, dtype=np.float64)
        bad = np.argwhere(got != ref) if d.kind == "exact" else np.argwhere(~(np.abs(got - ref) <= bound))
        if bad.size:
            at = tuple(bad[0])
            out.append("%s [%s]: %d elements of %s wrong, first %s = %r, expected %r" % (c["name"], d.kind, len(bad), what, at, got[at], ref[at]))
    return out
