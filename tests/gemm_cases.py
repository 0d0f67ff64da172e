"""The case list of svnet_gemm_f32's dispatch, stated once: tests/test_host_gemm_cases.py (CPU: the tier / variant queries, the bound's
own checks) and tests/test_hip_gemm_tiers.py (GPU: every case against float64) iterate the same table.

A case names the kernel family (svnet_gemm_tier) and template variant (svnet_gemm_variant) it is MEANT to reach, the descriptor's shape
(M, N, K as the descriptor has them), its strides, pointer offsets and options.  The expectations are written out by hand from the
dispatch rules of include/svnet_hip.h - a case that silently falls through to another kernel fails the query assertion before it runs.

Every case runs with two value kinds:
  int   small integers with zeros among them (B in +-1 / 0 or other bf16-exact values where b_exact), power-of-two scales and alpha,
        integer bias and initial C: every partial sum in any order stays below 2^24, so float32 arithmetic is exact whatever the
        summation order, the atomics or the bf16 splits do, and the result must equal the float64 product BIT FOR BIT.
  real  float32 standard normals with full mantissas, scales in [0.5, 1.5]; checked per element against
            |c_ij - ref_ij| <= C_BOUND * 2^-24 * ( |alpha cs_j| * sum_k |a_ik s_k b_kj| + |bias_j| + |C0_ij| )
        and the column sums against the sum over i of that right-hand side.

C_BOUND = 4 x the largest ratio |ref32 - ref64| / (2^-24 * bracket) that two float32 CPU references (torch's float32 matmul and a
sequential float32 accumulation over k) reach over the real cases of this list: C_MEASURED below, measured with measure_c().
"""
import zlib

import numpy as np
import torch

from svnet_amd import _lib

D = _lib.DEFINES
TN_TERN, TN_FP32, ROWS, ROWS_LDS = D["SVNET_GEMM_TN_TERN"], D["SVNET_GEMM_TN_FP32"], D["SVNET_GEMM_ROWS"], D["SVNET_GEMM_ROWS_LDS"]
ROWS_SPLIT, DOT, TILE = D["SVNET_GEMM_ROWS_SPLIT"], D["SVNET_GEMM_DOT"], D["SVNET_GEMM_TILE"]
FAMILY = {TN_TERN: "TN_TERN", TN_FP32: "TN_FP32", ROWS: "ROWS", ROWS_LDS: "ROWS_LDS", ROWS_SPLIT: "ROWS_SPLIT", DOT: "DOT", TILE: "TILE"}
E_ARG, E_UNSUPPORTED, E_WORKSPACE = D["SVNET_E_ARG"], D["SVNET_E_UNSUPPORTED"], D["SVNET_E_WORKSPACE"]
RED_SLICES = D["SVNET_RED_SLICES"]

C_MEASURED = 5.25       # largest float32-reference ratio over the real cases (measure_c(): 5.2499, the sequential sum of n_2_2, K = 1024)
C_BOUND = 4 * C_MEASURED
EPS24 = 2.0 ** -24

SENTINEL = -777.0       # what C holds before the call wherever the case does not accumulate, and in every gap between its elements
CONST_C0 = -3.0         # c0="const": the whole of C before an accumulating ternary call (cleared tiles must keep it)
PAD_VALUE = 12345.0     # what the padding of A and B holds: finite, and far from anything a sum of the operands gives


# ----------------------------------------------------------------------------- the variant packings of include/svnet_hip.h
def v_rows(nt, avec, deep, packed=0):
    return nt | avec << 4 | deep << 5 | packed << 6


def v_split(nj, w):
    return nj | w << 4


def v_tn(ip, jq):
    return ip | jq << 4


def v_tern(nq, ptiles, lds_reduce, compacted=0):
    return nq | ptiles << 4 | lds_reduce << 8 | compacted << 9


TERN_P = {10: (1, 1), 40: (2, 1), 70: (4, 0), 128: (4, 0), 150: (4, 0)}      # P -> (ptiles_per_block, lds_reduce)
ALL_EPI = ("a_scale", "col_scale", "bias", "mask", "col_sum", "alpha", "accumulate")

DEFAULTS = dict(
    a="rm", a_pad=0, a_gap=1, a_off=0,          # A: "rm" a_rs = a_gap K + a_pad, a_cs = a_gap;  "cm" a_rs = 1, a_cs = M + a_pad; a_off floats
    b="rm", b_pad=0,                            # B: "rm" b_rs = N + b_pad, b_cs = 1;  "cm" b_rs = 1, b_cs = K + b_pad
    c="rm", c_pad=0, c_gap=1,                   # C: "rm" ldc = c_gap N + c_pad, c_cs = c_gap;  "cm" ldc = 1, c_cs = M + c_pad
    b_exact=0, b_vals="sign",                   # b_exact values: "sign" (+-1 / 0) or "bf16" (other values exact in bf16)
    epi=(), ascale_off=0, split_k=0,            # epi: any of ALL_EPI
    ws=0, ws_off=0,                             # workspace: multiples of svnet_gemm_workspace_bytes(N, K), offset in bytes
    tern=0, tern_mask=0, c0="rand", no_nz=0,    # ternary A planes; c0: initial C under accumulate ("rand" or "const")
    rc=0,                                       # the code svnet_gemm_tier must return for a refusal (then nothing is launched)
)
CASES = []


def case(name, tier, variant, M, N, K, **opts):
    bad = set(opts) - set(DEFAULTS)
    assert not bad, bad
    assert all(c["name"] != name for c in CASES), name
    c = dict(DEFAULTS, name=name, tier=tier, variant=variant, M=M, N=N, K=K)
    c.update(opts)
    c["epi"] = tuple(c["epi"])
    CASES.append(c)


# ---- TILE: gemm_kernel, 64 x 64 x 16 tiles; variant = the number of K splits
case("t_1x1x1", TILE, 1, 1, 1, 1)
case("t_64x64x16", TILE, 1, 64, 64, 16)
case("t_63x65x15", TILE, 1, 63, 65, 15)
case("t_all_epi", TILE, 1, 130, 70, 33, epi=ALL_EPI)                           # mask of three words per column, M % 64 != 0
case("t_a_cm", TILE, 1, 70, 50, 40, a="cm")                                    # a_rs = 1 with K < 1024
case("t_pads_b_cm", TILE, 1, 65, 33, 20, a_pad=3, b="cm", b_pad=2, c_pad=5)
case("t_b_rm_pad", TILE, 1, 65, 33, 20, b_pad=3)
case("t_c_cm", TILE, 1, 40, 30, 20, c="cm")                                    # ldc = 1, c_cs = M
case("t_auto5_bias", TILE, 5, 100, 100, 300, epi=("bias",))                    # five chunks of 64, the last 44 long; bias once
case("t_auto5_mask_colsum", TILE, 5, 100, 100, 300, epi=("mask", "col_sum"))
case("t_auto5_acc", TILE, 5, 100, 100, 300, epi=("mask", "col_sum", "accumulate", "bias"))
case("t_split3_k40", TILE, 3, 50, 40, 40, split_k=3)                           # chunks 16, 16, 8
case("t_split7_k20", TILE, 2, 50, 40, 20, split_k=7)                           # collapses to 2
case("t_k0_bias", TILE, 1, 5, 7, 0, epi=("bias",))
case("t_k0", TILE, 1, 5, 7, 0)
case("t_m0", TILE, 1, 0, 5, 4)
case("t_n0", TILE, 1, 5, 0, 4, c_pad=4)                                          # (ldc = 0 would be an argument error)
case("t_exact_m15", TILE, 1, 15, 20, 16, b_exact=1)                            # pair: r_m16
case("t_exact_k7", TILE, 1, 20, 20, 7, b_exact=1)                              # pair: r_k8
case("t_mn8193", TILE, 1, 3, 2731, 128)                                        # pair: d_mn8192
case("t_dot_mask", TILE, 4, 32, 40, 256, epi=("mask",))                        # pair: d_32x40x256
case("t_dot_split2", TILE, 2, 32, 40, 256, split_k=2)
case("t_tn_k1023", TILE, 16, 100, 100, 1023, a="cm")                           # pair: n_k1024
case("t_tn_m4097", TILE, 16, 4097, 8, 1024, a="cm")                            # pair: n_2_1

# ---- DOT: gemm_dot_kernel, one wave per output
case("d_32x40x256", DOT, 0, 32, 40, 256)
case("d_1x1x128", DOT, 0, 1, 1, 128)
for _k in (128, 129, 191, 192, 193, 255):                                      # the pair loop and its tail
    case("d_k%d" % _k, DOT, 0, 3, 5, _k)
case("d_mn8192", DOT, 0, 64, 128, 128)
case("d_epi_gaps", DOT, 0, 7, 9, 193, epi=("a_scale", "col_scale", "bias", "alpha", "accumulate"), a_gap=2, a_pad=1, c_gap=3, c_pad=2)
case("d_b_cm", DOT, 0, 7, 9, 193, b="cm", b_pad=1, epi=("bias",))
case("d_split_m1023", DOT, 0, 1023, 8, 128, ws=3)                              # too few rows for ROWS_SPLIT; pair: s_m1024_dotsized

# ---- ROWS: mfma_rows_kernel<NT, AVEC, DEEP>, b_exact
case("r_16x1x8", ROWS, v_rows(1, 1, 0), 16, 1, 8, b_exact=1)
case("r_m16", ROWS, v_rows(1, 1, 0), 16, 20, 16, b_exact=1)
case("r_k8", ROWS, v_rows(1, 1, 0), 20, 20, 8, b_exact=1)
case("r_17x33x9", ROWS, v_rows(1, 0, 0), 17, 33, 9, b_exact=1)
case("r_nt2", ROWS, v_rows(2, 1, 0), 513, 33, 16, b_exact=1)
case("r_nt4", ROWS, v_rows(4, 1, 0), 513, 65, 24, b_exact=1)
case("r_nt8_deep", ROWS, v_rows(8, 1, 1), 513, 129, 72, b_exact=1)
case("r_640x257x136", ROWS, v_rows(8, 1, 1), 640, 257, 136, b_exact=1)         # two column groups, two K chunks
case("r_130x300x64", ROWS, v_rows(1, 1, 0), 130, 300, 64, b_exact=1)           # M <= 512: ten 32-column groups
for _k, _v in ((64, v_rows(1, 1, 0)), (65, v_rows(1, 0, 1)), (128, v_rows(1, 1, 1)), (129, v_rows(1, 0, 1)), (264, v_rows(1, 1, 1))):
    case("r_k%d" % _k, ROWS, _v, 70, 40, _k, b_exact=1)
case("r_a_off1", ROWS, v_rows(1, 0, 0), 64, 40, 16, b_exact=1, a_off=1)        # K % 8 == 0, pointer unaligned
case("r_pads_vec", ROWS, v_rows(1, 1, 0), 64, 40, 16, b_exact=1, a_pad=4, c_pad=3)
case("r_pads_scalar", ROWS, v_rows(1, 0, 0), 64, 40, 16, b_exact=1, a_pad=1, c_pad=3)
case("r_b_cm", ROWS, v_rows(1, 1, 0), 70, 40, 24, b_exact=1, b="cm", b_pad=2)
case("r_b_bf16", ROWS, v_rows(1, 1, 0), 70, 40, 24, b_exact=1, b_vals="bf16")
case("r_packed_b_rm", ROWS, v_rows(1, 1, 0, 1), 200, 40, 24, b_exact=1, ws=1)
case("r_packed_b_cm", ROWS, v_rows(1, 1, 0, 1), 200, 40, 24, b_exact=1, ws=1, b="cm")
case("r_packed_misaligned_ws", ROWS, v_rows(1, 1, 0, 0), 200, 40, 24, b_exact=1, ws=1, ws_off=8)     # not packed, still served
case("r_packed_m4095", ROWS, v_rows(8, 0, 1, 1), 4095, 257, 68, b_exact=1, ws=1)                     # pair: l_m4096
for _e in ALL_EPI:
    case("r_vec_" + _e, ROWS, v_rows(1, 1, 0), 70, 40, 16, b_exact=1, epi=(_e,))
    case("r_scalar_" + _e, ROWS, v_rows(1, 0, 0), 70, 40, 17, b_exact=1, epi=(_e,))
case("r_vec_all_epi", ROWS, v_rows(2, 1, 1), 600, 40, 72, b_exact=1, epi=ALL_EPI)
case("r_scalar_all_epi", ROWS, v_rows(1, 0, 0), 70, 40, 17, b_exact=1, epi=ALL_EPI)
case("r_persist_single", ROWS, v_rows(1, 1, 0), 2048 * 128 + 130, 8, 8, b_exact=1, epi=("col_sum",))  # B kept, column partials carried
case("r_persist_chunks", ROWS, v_rows(1, 1, 1), 4096 * 128 + 130, 8, 136, b_exact=1)                 # the multi-chunk cap

# ---- ROWS_LDS: mfma_rows2_kernel<1, aligned>, B packed into the workspace
case("l_4096x129x64", ROWS_LDS, 1, 4096, 129, 64, b_exact=1, ws=1)
case("l_m4096", ROWS_LDS, 1, 4096, 257, 68, b_exact=1, ws=1)
case("l_4097x257x68", ROWS_LDS, 1, 4097, 257, 68, b_exact=1, ws=1)             # ragged M, two 256-column groups
case("l_4100x130x83", ROWS_LDS, 0, 4100, 130, 83, b_exact=1, ws=1)             # odd K: scalar A loads
case("l_ascale_off1", ROWS_LDS, 0, 4096, 129, 64, b_exact=1, ws=1, epi=("a_scale",), ascale_off=1)
case("l_lda", ROWS_LDS, 1, 4096, 129, 64, b_exact=1, ws=1, a_pad=4)
case("l_all_epi", ROWS_LDS, 1, 4097, 130, 64, b_exact=1, ws=1, epi=ALL_EPI)
case("l_scalar_all_epi", ROWS_LDS, 0, 4100, 130, 83, b_exact=1, ws=1, epi=ALL_EPI, c_pad=1)

# ---- ROWS_SPLIT: mfma_rows3_kernel<NJ, W>, general B, a workspace of three packed pieces
for _n, _nj in ((64, 1), (65, 2), (128, 2), (129, 4)):
    case("s_n%d" % _n, ROWS_SPLIT, v_split(_nj, 4), 1024, _n, 16, ws=3)
case("s_a_off1", ROWS_SPLIT, v_split(1, 1), 1024, 64, 16, ws=3, a_off=1)
case("s_a_off2", ROWS_SPLIT, v_split(1, 2), 1024, 64, 16, ws=3, a_off=2)
case("s_k19", ROWS_SPLIT, v_split(1, 1), 1024, 64, 19, ws=3)
case("s_epi", ROWS_SPLIT, v_split(2, 4), 1025, 65, 24, ws=3, epi=("alpha", "bias", "accumulate"), c_pad=2)
case("s_m1024_dotsized", ROWS_SPLIT, v_split(1, 4), 1024, 8, 128, ws=3)
case("t_split_m1023", TILE, 1, 1023, 64, 16, ws=3)                             # pair: s_n64
case("x_split_misaligned_ws", ROWS_SPLIT, 0, 1024, 64, 16, ws=3, ws_off=8, rc=E_WORKSPACE)

# ---- TN_FP32: mfma_tn2_kernel<IP, JQ>; a_rs = 1, b_cs = 1, K >= 1024
case("n_2_2", TN_FP32, v_tn(2, 2), 520, 840, 1024, a="cm")
case("n_2_1", TN_FP32, v_tn(2, 1), 4096, 8, 1024, a="cm")
case("n_1_2", TN_FP32, v_tn(1, 2), 8, 4096, 1024, a="cm")
case("n_2_1_fourth", TN_FP32, v_tn(2, 1), 129, 1025, 1024, a="cm")
case("n_1_1", TN_FP32, v_tn(1, 1), 10, 20, 1024, a="cm")
case("n_1_1_65", TN_FP32, v_tn(1, 1), 65, 65, 1024, a="cm")
case("n_k1024", TN_FP32, v_tn(1, 1), 100, 100, 1024, a="cm")
case("n_k1025", TN_FP32, v_tn(1, 1), 10, 20, 1025, a="cm")                     # the slab tails
case("n_k1055", TN_FP32, v_tn(1, 1), 65, 65, 1055, a="cm")
case("n_alpha_acc", TN_FP32, v_tn(1, 1), 65, 65, 1024, a="cm", epi=("alpha", "accumulate"))
case("n_c_cm_lda", TN_FP32, v_tn(1, 1), 65, 65, 1025, a="cm", a_pad=3, c="cm", c_pad=1, b_pad=2)

# ---- TN_TERN: mfma_tn_tern_kernel<NQ>; ternary A planes.  Q = M, P = N, rows = K
for _q, _p, _rows, _nq, _o in ((32, 10, 1, 1, {}), (33, 40, 63, 2, {}), (64, 70, 64, 2, dict(epi=("alpha",))), (65, 128, 65, 4, {}),
                               (128, 150, 255, 4, dict(c="cm")), (129, 10, 256, 5, dict(b_pad=3)), (160, 40, 257, 5, dict(c="cm", c_pad=2)),
                               (161, 70, 1000, 5, {}), (320, 128, 300, 5, dict(epi=("alpha", "accumulate"))), (505, 150, 130, 5, {}),
                               (64, 10, 1000, 2, dict(epi=("accumulate",)))):
    case("q_%dx%dx%d" % (_q, _p, _rows), TN_TERN, v_tern(_nq, *TERN_P[_p]), _q, _p, _rows, tern=1, **_o)
_ACC = dict(tern=1, epi=("accumulate",), c0="const")
case("q_mask_zero", TN_TERN, v_tern(5, 2, 1), 320, 40, 100, tern_mask=0, **_ACC)
case("q_mask_ones", TN_TERN, v_tern(5, 2, 1), 320, 40, 100, tern_mask=0xFFFFFFFF, **_ACC)
case("q_mask_compacted", TN_TERN, v_tern(5, 2, 1, 1), 320, 40, 100, tern_mask=0x205, **_ACC)          # tiles 0, 2, 9
case("q_mask_compacted_store", TN_TERN, v_tern(5, 2, 1, 1), 320, 40, 100, tern=1, tern_mask=0x205)    # cleared tiles are zero-filled
case("q_mask_eight", TN_TERN, v_tern(5, 2, 1), 320, 40, 100, tern_mask=0x3B7, **_ACC)                 # more than NQ live tiles
case("q_mask_past_end", TN_TERN, v_tern(5, 2, 1, 1), 320, 40, 100, tern_mask=0x5 | 1 << 20, **_ACC)   # bit 20: no such tile
case("q_mask_tile15", TN_TERN, v_tern(5, 2, 1), 512, 40, 70, tern_mask=0x8001, **_ACC)                # tile 15 does not fit the 4-bit list
case("q_mask_tile14", TN_TERN, v_tern(5, 2, 1, 1), 512, 40, 70, tern_mask=0x4001, **_ACC)
case("q_mask_tile15_p70", TN_TERN, v_tern(5, 4, 0), 505, 70, 130, tern_mask=0x8003, **_ACC)
case("x_tern_mask_q1056", TN_TERN, 0, 1056, 40, 70, tern=1, tern_mask=0x3, rc=E_UNSUPPORTED)
case("x_tern_b_cm", TN_TERN, 0, 64, 40, 70, tern=1, b="cm", rc=E_UNSUPPORTED)
case("x_tern_bias", TN_TERN, 0, 64, 40, 70, tern=1, epi=("bias",), rc=E_UNSUPPORTED)
case("x_tern_no_nz", TN_TERN, 0, 64, 40, 70, tern=1, no_nz=1, rc=E_ARG)

# the two sides of every dispatch boundary (the first name lies below it)
BOUNDARY_PAIRS = [
    ("t_exact_m15", "r_m16"),                   # M = 15 / 16 with b_exact
    ("t_exact_k7", "r_k8"),                     # K = 7 / 8 with b_exact
    ("t_tn_k1023", "n_k1024"),                  # K = 1023 / 1024 with a_rs = 1, b_cs = 1
    ("d_mn8192", "t_mn8193"),                   # M * N = 8192 / 8193
    ("r_packed_m4095", "l_m4096"),              # M = 4095 / 4096 with a workspace
    ("t_split_m1023", "s_n64"),                 # M = 1023 / 1024 with a 3x workspace
    ("d_split_m1023", "s_m1024_dotsized"),
    ("n_2_1", "t_tn_m4097"),                    # M = 4096 / 4097 with a_rs = 1, b_cs = 1
    ("r_k64", "r_k65"),                         # DEEP
    ("q_mask_tile14", "q_mask_tile15"),         # the compacted tile list holds tiles 0 .. 14
]
SPLIT_FAMILIES = (TN_TERN, TN_FP32, ROWS, ROWS_LDS, ROWS_SPLIT)         # operands split into bf16 pieces
RUN_CASES = [c for c in CASES if c["rc"] == 0]
REFUSALS = [c for c in CASES if c["rc"] != 0]
KINDS = ("int", "real")


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# ----------------------------------------------------------------------------- layout
def layout(c):
    """Strides of the descriptor and the length (float32 elements) of each operand's storage, pointer offsets included."""
    M, N, K = c["M"], c["N"], c["K"]
    if c["a"] == "rm":
        a_rs, a_cs = c["a_gap"] * K + c["a_pad"], c["a_gap"]
    else:
        a_rs, a_cs = 1, M + c["a_pad"]
    b_rs, b_cs = (N + c["b_pad"], 1) if c["b"] == "rm" else (1, K + c["b_pad"])
    if c["c"] == "rm":
        ldc, c_cs = c["c_gap"] * N + c["c_pad"], c["c_gap"]
    else:
        ldc, c_cs = 1, M + c["c_pad"]

    def extent(n0, s0, n1, s1):
        return (max(n0, 1) - 1) * s0 + (max(n1, 1) - 1) * s1 + 1

    # whole leading dimensions: a row's padding belongs to the storage
    a_len = (max(M, 1) * a_rs if c["a"] == "rm" else max(K, 1) * a_cs)
    b_len = (max(K, 1) * b_rs if c["b"] == "rm" else max(N, 1) * b_cs)
    c_len = (max(M, 1) * ldc if c["c"] == "rm" else max(N, 1) * c_cs)
    a_len, b_len, c_len = max(a_len, 1), max(b_len, 1), max(c_len, 1)             # (K = 0 gives a zero row stride)
    assert a_len >= extent(M, a_rs, K, a_cs) and b_len >= extent(K, b_rs, N, b_cs) and c_len >= extent(M, ldc, N, c_cs)
    return dict(a_rs=a_rs, a_cs=a_cs, b_rs=b_rs, b_cs=b_cs, ldc=ldc, c_cs=c_cs, a_len=c["a_off"] + max(a_len, 1), b_len=max(b_len, 1),
                c_len=max(c_len, 1))


def workspace_bytes(c):
    return c["ws"] * _lib.lib().svnet_gemm_workspace_bytes(c["N"], c["K"])


def words(n):
    return (n + 63) // 64


def fill_desc(c, ptr, kind="int"):
    """The descriptor of a case over the addresses ptr[name] of its buffers' storage (a_off / ascale_off / ws_off are applied here)."""
    L = layout(c)
    d = _lib.GemmDesc()
    d.M, d.N, d.K = c["M"], c["N"], c["K"]
    if c["tern"]:
        d.a_sign = ptr["a_sign"]
        d.a_nz = None if c["no_nz"] else ptr["a_nz"]
    else:
        d.A, d.a_rs, d.a_cs = ptr["A"] + 4 * c["a_off"], L["a_rs"], L["a_cs"]
    d.B, d.b_rs, d.b_cs = ptr["B"], L["b_rs"], L["b_cs"]
    d.b_exact = c["b_exact"]
    d.C, d.ldc, d.c_cs = ptr["C"], L["ldc"], L["c_cs"]
    d.alpha = alpha_of(c, kind)
    if "a_scale" in c["epi"]:
        d.a_scale = ptr["a_scale"] + 4 * c["ascale_off"]
    if "col_scale" in c["epi"]:
        d.col_scale = ptr["col_scale"]
    if "bias" in c["epi"]:
        d.bias = ptr["bias"]
    if "mask" in c["epi"]:
        d.mask = ptr["mask"]
    if "col_sum" in c["epi"]:
        d.col_sum = ptr["col_sum"]
    d.split_k = c["split_k"]
    d.accumulate = int("accumulate" in c["epi"])
    d.tern_tile_mask = c["tern_mask"]
    if c["ws"]:
        d.workspace, d.workspace_bytes = ptr["ws"] + c["ws_off"], workspace_bytes(c)
    return d


def fake_pointers(c):
    """Non-null addresses with the case's real alignments (storage 256-byte aligned, as a device allocation is); never dereferenced."""
    names = ("A", "B", "C", "a_scale", "col_scale", "bias", "mask", "col_sum", "a_sign", "a_nz", "ws")
    return {n: 0x7F0000000000 + 0x10000000 * i for i, n in enumerate(names)}


def alpha_of(c, kind):
    if "alpha" not in c["epi"]:
        return 1.0
    return 0.5 if kind == "int" else 0.8125


# ----------------------------------------------------------------------------- values
class Data:
    pass


def _view(store, off, shape, strides):
    return np.lib.stride_tricks.as_strided(store[off:], shape, tuple(4 * s for s in strides))


def build(c, kind):
    """The operands of a case as float32 storage arrays (what the device gets) with strided views of the logical matrices into them."""
    M, N, K = c["M"], c["N"], c["K"]
    L = layout(c)
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (c["name"], kind)).encode()))
    x = Data()
    x.kind, x.alpha = kind, alpha_of(c, kind)

    def values(shape, lo, hi):
        if kind == "int":
            return rng.integers(lo, hi + 1, size=shape).astype(np.float32)
        return rng.standard_normal(size=shape, dtype=np.float32)

    def scales(n):
        if kind == "int":
            return rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=n)
        return rng.uniform(0.5, 1.5, size=n).astype(np.float32)

    if c["tern"]:
        T = rng.integers(-1, 2, size=(M, K)).astype(np.int8)                    # tern(i, k)
        x.T = T
        wk = words(K)
        bit = (np.uint64(1) << (np.arange(K, dtype=np.uint64) & np.uint64(63)))[None, :]
        nz = np.zeros((wk, M), np.uint64)
        sg = np.zeros((wk, M), np.uint64)
        dirty = rng.integers(0, 2, size=(M, K)).astype(bool)                    # sign bits under a clear non-zero bit: to be ignored
        for w in range(wk):
            ks = slice(64 * w, min(K, 64 * w + 64))
            nz[w] = np.bitwise_or.reduce(np.where(T[:, ks] != 0, bit[:, ks], np.uint64(0)), axis=1)
            sg[w] = np.bitwise_or.reduce(np.where((T[:, ks] > 0) | ((T[:, ks] == 0) & dirty[:, ks]), bit[:, ks], np.uint64(0)), axis=1)
        x.a_nz, x.a_sign = nz.ravel(), sg.ravel()
        x.A = T.astype(np.float32)
        x.A_store = None
    else:
        x.A_store = np.full(L["a_len"], PAD_VALUE, np.float32)
        x.A = _view(x.A_store, c["a_off"], (M, K), (L["a_rs"], L["a_cs"]))
        x.A[...] = values((M, K), -4, 4)
    x.B_store = np.full(L["b_len"], PAD_VALUE, np.float32)
    x.B = _view(x.B_store, 0, (K, N), (L["b_rs"], L["b_cs"]))
    if c["b_exact"]:                                                            # exact in bf16, in both kinds
        pool = [-1.0, 0.0, 1.0] if c["b_vals"] == "sign" else [0.5, -3.0, 0.0, 1.0, -1.0, 2.0, -0.25, 1.5]
        x.B[...] = rng.choice(np.array(pool, np.float32), size=(K, N))
    else:
        x.B[...] = values((K, N), -3, 3)
    x.C_store = np.full(L["c_len"], CONST_C0 if c["c0"] == "const" else SENTINEL, np.float32)
    x.C0 = _view(x.C_store, 0, (M, N), (L["ldc"], L["c_cs"]))
    x.written = np.zeros(L["c_len"], bool)
    _w = np.lib.stride_tricks.as_strided(x.written, (M, N), (L["ldc"], L["c_cs"]))
    _w[...] = True
    if "accumulate" in c["epi"] and c["c0"] == "rand":
        x.C0[...] = values((M, N), -8, 8)
    x.a_scale = x.col_scale = x.bias = x.mask = None
    if "a_scale" in c["epi"]:
        x.a_scale_store = np.full(K + c["ascale_off"], PAD_VALUE, np.float32)
        x.a_scale = x.a_scale_store[c["ascale_off"]:]
        x.a_scale[...] = scales(K)
    if "col_scale" in c["epi"]:
        x.col_scale = scales(N)
    if "bias" in c["epi"]:
        x.bias = values(N, -8, 8)
    if "mask" in c["epi"]:
        x.mask_bits = rng.integers(0, 2, size=(M, N)).astype(bool)
        mw = np.zeros((words(M), N), np.uint64)
        for i in range(M):
            mw[i >> 6] |= np.where(x.mask_bits[i], np.uint64(1) << np.uint64(i & 63), np.uint64(0))
        x.mask = mw.ravel()
    return x


def live_rows(c):
    """Ternary cases: which output rows i (column tiles of the kernel) the tile mask leaves live."""
    M = c["M"]
    m = c["tern_mask"] or 0xFFFFFFFF
    if m == 0xFFFFFFFF:
        return np.ones(M, bool)
    t = np.arange(M) // 32
    return (t < 32) & (((m >> np.minimum(t, 31)) & 1) == 1)


class Ref:
    pass


def reference(c, x, chunk=65536, A=None, B=None):
    """float64: C (the expected values), mag (the bracket of the bound, per element), col_sum / col_mag.  A / B: other operand values
    than the case's own (the teeth checks: a product that lost precision)."""
    M, N, K = c["M"], c["N"], c["K"]
    A = x.A if A is None else A
    B = x.B if B is None else B
    r = Ref()
    r.C = np.empty((M, N))
    r.mag = np.empty((M, N))
    B64 = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64))
    s = None if x.a_scale is None else x.a_scale.astype(np.float64)
    cs = np.ones(N) if x.col_scale is None else x.col_scale.astype(np.float64)
    bias = np.zeros(N) if x.bias is None else x.bias.astype(np.float64)
    acc = "accumulate" in c["epi"]
    live = live_rows(c) if c["tern"] else None
    for i0 in range(0, M, chunk):
        sl = slice(i0, min(M, i0 + chunk))
        a = np.ascontiguousarray(A[sl], dtype=np.float64)
        if s is not None:
            a = a * s
        a = torch.from_numpy(a)
        prod = (a @ B64).numpy() * (x.alpha * cs)
        mag = (a.abs() @ B64.abs()).numpy() * np.abs(x.alpha * cs)
        v = prod + bias
        if x.mask is not None:
            v = np.where(x.mask_bits[sl], v, 0.0)
        r.C[sl], r.mag[sl] = v, mag + np.abs(bias)
    r.col_sum = r.C.sum(axis=0) if "col_sum" in c["epi"] else None
    c0 = x.C0.astype(np.float64)
    if live is not None:                                                        # cleared tiles: not part of the product at all
        r.C[~live], r.mag[~live] = 0.0, 0.0
    if acc:                                                                     # (without it the whole of C is zero-filled first: cleared tiles read 0)
        r.C += c0
        r.mag += np.abs(c0)
    r.col_mag = r.mag.sum(axis=0)
    return r


def refs_f32(c, x):
    """The two float32 CPU references the bound is calibrated on: torch's float32 matmul, and a sequential float32 sum over k."""
    M, N, K = c["M"], c["N"], c["K"]
    f = np.float32
    a = np.ascontiguousarray(x.A, dtype=f)
    if x.a_scale is not None:
        a = a * x.a_scale
    b = np.ascontiguousarray(x.B, dtype=f)
    mm = (torch.from_numpy(a) @ torch.from_numpy(b)).numpy()
    seq = np.zeros((M, N), f)
    for k in range(K):
        seq += a[:, k:k + 1] * b[k:k + 1, :]
    out = []
    for p in (mm, seq):
        v = p * f(x.alpha)
        if x.col_scale is not None:
            v = v * x.col_scale
        if x.bias is not None:
            v = v + x.bias
        if x.mask is not None:
            v = np.where(x.mask_bits, v, f(0))
        col = v.sum(axis=0, dtype=f) if "col_sum" in c["epi"] else None
        if c["tern"]:
            v[~live_rows(c)] = 0
        if "accumulate" in c["epi"]:
            v = v + x.C0
        out.append((v.astype(f), col))
    return out


def truncated(a):
    """float32 values cut to 16 significant bits: what a product computes that drops the third bf16 piece of an operand."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)


def expected_store(c, x, r):
    """The whole storage of C after a correct call, in float32."""
    L = layout(c)
    out = x.C_store.copy()
    _view(out, 0, (c["M"], c["N"]), (L["ldc"], L["c_cs"]))[...] = r.C.astype(np.float32)
    return out


def col_sum_of(buf, N):
    """Totals of a sliced accumulator of N sums whose slices the kernel filled (SVNET_SLICED_LEN: [N totals | slices x N | 2])."""
    return np.asarray(buf[N:N + RED_SLICES * N], dtype=np.float64).reshape(RED_SLICES, N).sum(axis=0)


def ratios(c, x, r, C, col_sum=None):
    """(largest |C - ref| / (2^-24 bracket), its index, the same for the column sums): what C_BOUND bounds.  0 / 0 counts as 0."""
    err = np.abs(np.asarray(C, dtype=np.float64) - r.C)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (EPS24 * r.mag))
    q = np.nan_to_num(q, nan=np.inf)
    at = np.unravel_index(int(q.argmax()), q.shape) if q.size else (0, 0)
    worst = float(q[at]) if q.size else 0.0
    cw = 0.0
    if r.col_sum is not None and c["N"]:
        ce = np.abs(np.asarray(col_sum, dtype=np.float64) - r.col_sum)
        with np.errstate(divide="ignore", invalid="ignore"):
            cq = np.nan_to_num(np.where(ce == 0, 0.0, ce / (EPS24 * r.col_mag)), nan=np.inf)
        cw = float(cq.max())
    return worst, at, cw


def failures(c, x, r, C_store, col_sum=None, bound=C_BOUND):
    """Why a result (the whole storage of C after the call, the column totals) is not the case's reference; [] when it is.
    int kind: bit for bit.  real kind: the per-element bound.  Both: every element of the storage outside C(i, j) keeps its value."""
    out = []
    L = layout(c)
    tag = "%s [%s %s variant %d]" % (c["name"], x.kind, FAMILY[c["tier"]], c["variant"])
    C_store = np.asarray(C_store)
    gaps = np.flatnonzero(~x.written & (C_store != x.C_store))
    if gaps.size:
        out.append("%s: %d elements outside C(i, j) were written, first at offset %d: %r" % (tag, gaps.size, gaps[0], C_store[gaps[0]]))
    C = _view(C_store, 0, (c["M"], c["N"]), (L["ldc"], L["c_cs"]))
    if x.kind == "int":
        bad = np.argwhere(C.astype(np.float64) != r.C)
        if bad.size:
            i, j = bad[0]
            out.append("%s: %d of %d elements differ from the exact product, first C(%d, %d) = %r, expected %r"
                       % (tag, len(bad), C.size, i, j, C[i, j], r.C[i, j]))
        if r.col_sum is not None and np.any(np.asarray(col_sum, dtype=np.float64) != r.col_sum):
            j = int(np.flatnonzero(np.asarray(col_sum, dtype=np.float64) != r.col_sum)[0])
            out.append("%s: col_sum[%d] = %r, expected %r" % (tag, j, col_sum[j], r.col_sum[j]))
        return out
    worst, at, cw = ratios(c, x, r, C, col_sum)
    if worst > bound:
        out.append("%s: worst element C(%d, %d) = %r, expected %r: %.1f x 2^-24 of its bracket %.4g, bound %.1f"
                   % (tag, at[0], at[1], C[at], r.C[at], worst, r.mag[at], bound))
    if cw > bound:
        out.append("%s: column sums off by %.1f x 2^-24 of their bracket, bound %.1f" % (tag, cw, bound))
    return out


def measure_c(verbose=False):
    """The largest ratio the float32 CPU references reach over the real cases (C_MEASURED)."""
    top = (0.0, None)
    for c in RUN_CASES:
        if c["M"] == 0 or c["N"] == 0:
            continue
        x = build(c, "real")
        r = reference(c, x)
        for which, (v, col) in zip(("matmul", "sequential"), refs_f32(c, x)):
            worst, _, cw = ratios(c, x, r, v, col)
            if verbose:
                print("%-28s %-10s %.3f %.3f" % (c["name"], which, worst, cw))
            top = max(top, (worst, c["name"] + "/" + which), (cw, c["name"] + "/" + which + "/col_sum"))
    return top


if __name__ == "__main__":
    print(measure_c(verbose=True))
