"""The shape envelope of the two fused edge-level blocks as ONE case table, shared by the GPU tests (tests/test_hip_block_envelope.py: the
kernels against the float64 oracle) and the CPU tests (tests/test_host_block_envelope.py: which instantiation each case reaches, that the
table reaches every instantiation there is, and that the oracle alone is well conditioned on every case).

An edge-block case is (tag, (Cs, Cv), (Os, Ov), B, N, k, expect): point-table widths in -> out, clouds, points per cloud, neighbours;
expect = {"fwd", "bwd", "wgrad"}: the values svnet_edgeblock_fwd_tier / svnet_edgeblock_bwd_tier / svnet_edgeblock_wgrad_tier must return
(include/svnet_hip.h: fwd 1 = the two-edge kernel, 100 + 10 OP + NARROW = edgeblock_fwd_kernel<OP, NARROW>; bwd 100 NKS + NC2 =
edgeblock_bwd_kernel<0, NKS, NC2>; wgrad 2 = mfma_tn_aff2, 1 = mfma_tn_tern<5> with the affine operand, -1 = dn_out + the ternary GEMM),
or None for a shape the fused block refuses (it then runs layer-wise and must still match the oracle).
A first-layer case is (tag, nc, (Os, Ov), B, N, k, tier) with tier = svnet_xyzblock_tier's 10 NC + EPI.
"""
import contextlib
import io
from collections import OrderedDict

import torch

from oracle import sv_ref
from svnet_amd._lib import DEFINES
from tests.golden import cases as C
from tests.golden import harness as H

TWO = DEFINES["SVNET_EDGE_FWD_TWO"]
OUT_RTOL = 1e-4         # outputs and running statistics (tests/common.py compare_case scaling)
GRAD_RTOL = 1e-3        # gradients: the project's north-star tolerance (tests/test_hip_train_parity.py)
MAX_EDGES = 25000       # every case stays at E = B*N*k below this: a few seconds at the most, float64 oracle included


def _t(fwd, bwd, wgrad):
    return {"fwd": fwd, "bwd": bwd, "wgrad": wgrad}


_N = ((32, 10), (64, 21))       # the narrow sweep layer: edgeblock_fwd_kernel<1, true>, edgeblock_bwd_kernel<0, 4, 20>
_W = ((64, 21), (128, 42))      # the wide sweep layer: edgeblock_fwd_kernel<2, false>, edgeblock_bwd_kernel<0, 8, 44>, all ten column tiles in use
SWEEP_K = (2, 3, 5, 8, 9, 16, 31, 32, 33, 63, 64)
# the wide layer's weight-gradient kernel at B = 2, N = 66: E = 132 k is a whole number of 32-row slabs only for k % 8 == 0
_W66 = {2: -1, 3: -1, 5: -1, 8: 2, 9: 1, 16: 2, 31: 1, 32: 2, 33: 1, 63: 1, 64: 2}

EDGE_CASES = [
    # ---- backward tile kernel: NC2 x NKS
    ("bwd_2_24", (32, 12), (32, 12), 2, 70, 9, _t(TWO, 224, 1)),
    ("bwd_4_24", (33, 11), (64, 12), 2, 70, 9, _t(110, 424, 1)),
    ("bwd_8_24", (32, 12), (128, 24), 2, 40, 8, _t(121, 824, 1)),
    ("bwd_8_20", (64, 10), (128, 20), 1, 72, 20, _t(120, 820, 1)),
    ("bwd_2_44", (32, 16), (32, 16), 2, 40, 5, _t(TWO, 244, -1)),
    ("bwd_2_48", (48, 24), (32, 16), 2, 64, 8, _t(110, 248, 1)),
    ("bwd_4_48", (64, 24), (64, 24), 1, 96, 12, _t(110, 448, 1)),
    ("bwd_8_48", (64, 24), (128, 40), 1, 40, 10, _t(120, 848, 1)),
    # ---- the one-edge form of phase C (NC2 = 0)
    ("one_cv2_os8_k2", (8, 2), (8, 2), 2, 40, 2, _t(TWO, 200, -1)),
    ("one_cv1_os16_k3", (5, 1), (16, 3), 3, 33, 3, _t(TWO, 200, -1)),
    ("one_3cv_gt_2cs", (16, 16), (64, 33), 2, 65, 33, _t(111, 400, 1)),
    ("one_every_limit", (64, 32), (128, 64), 1, 64, 64, _t(120, 800, 2)),
    ("one_cv25", (20, 25), (64, 20), 1, 90, 11, _t(110, 400, 1)),
    # ---- forward pairs
    ("fwd_1_wide", (64, 21), (64, 21), 2, 80, 7, _t(110, 444, -1)),
    ("fwd_2_narrow", (32, 10), (128, 42), 2, 80, 20, _t(121, 820, 1)),
    ("fwd_narrow_ov33", (32, 10), (32, 33), 2, 96, 6, _t(111, 220, -1)),
]
# ---- k sweep: N = 66 makes N*k % 32 != 0 for odd k; N = 64 adds the whole-tile case
EDGE_CASES += [("k%d_narrow" % k, _N[0], _N[1], 2, 66, k, _t(111, 420, -1 if k < 8 else 1)) for k in SWEEP_K]
EDGE_CASES += [("k%d_wide" % k, _W[0], _W[1], 2, 66, k, _t(120, 844, _W66[k])) for k in SWEEP_K]
EDGE_CASES += [("k%d_narrow_n64" % k, _N[0], _N[1], 2, 64, k, _t(111, 420, 1)) for k in (16, 32, 64)]
EDGE_CASES += [("k%d_wide_n64" % k, _W[0], _W[1], 2, 64, k, _t(120, 844, 2)) for k in (16, 32, 64)]
EDGE_CASES += [
    # ---- XCD tile order of the backward tile kernel: B % 8 == 0 and N*k % 32 == 0
    ("xcd_b8", (32, 10), (32, 10), 8, 64, 16, _t(TWO, 220, 1)),
    ("xcd_b16_k6", (64, 21), (128, 42), 16, 48, 6, _t(120, 844, -1)),      # (E % 32 == 0, Os = 128, ten tiles - but k < 8: dn_out + ternary GEMM)
    # ---- more than one point per wave (B*N > 4096); N = 131: two points per wave and a last wave with one
    ("waves_n130", (32, 10), (32, 10), 40, 130, 4, _t(TWO, 220, -1)),
    ("waves_n131", (32, 10), (32, 10), 40, 131, 4, _t(TWO, 220, -1)),
    # ---- refused shapes: layer-wise, same oracle
    ("refused_os24", (32, 10), (24, 10), 2, 40, 6, None),
    ("refused_k65", (32, 10), (32, 10), 1, 70, 65, None),
    ("refused_cs65", (65, 10), (32, 10), 2, 40, 6, None),
    ("refused_cv33", (32, 33), (32, 10), 2, 40, 6, None),
    ("refused_ov65", (32, 10), (32, 65), 2, 40, 6, None),
]

XYZ_OUT_DIMS = ((64, 21), (33, 40), (64, 64), (32, 33), (8, 3))
XYZ_SIZES = ((2, 96, 6), (1, 64, 64), (40, 130, 4))


def _xyz_tier(nc, out_dims):
    return 10 * nc + (2 if out_dims == (8, 3) else 1)        # (8,3) is the only out_dims of the list with both widths <= 32


XYZ_CASES = [("nc%d_%dx%d_b%dn%dk%d" % ((nc,) + od + sz), nc, od, sz[0], sz[1], sz[2], _xyz_tier(nc, od))
             for nc in (2, 3) for od in XYZ_OUT_DIMS for sz in XYZ_SIZES]
# B*N > 4096 with an odd N: the backward's two points per wave and a last wave with one
XYZ_CASES += [("nc2_64x21_b40n131k4", 2, (64, 21), 40, 131, 4, 21), ("nc3_8x3_b40n131k4", 3, (8, 3), 40, 131, 4, 32)]

# Cases whose first draw of inputs put a sign decision on a knife edge of rounding IN THE ORACLE (its fp32 and float64 runs took one
# |s_v + beta| ~ 1e-7 different ways: tests/test_host_block_envelope.py test_edge_oracle_is_well_conditioned measured 8.9e-3 on dx1 of
# xcd_b16_k6): another draw of the same shape, never a looser bound.
REDRAWN = {"xcd_b16_k6": 1}


def _stream(tag):
    return "envelope/%s" % tag + ("#%d" % REDRAWN[tag] if tag in REDRAWN else "")


assert all(c[3] * c[4] * c[5] <= MAX_EDGES for c in EDGE_CASES) and all(c[3] * c[4] * c[5] <= MAX_EDGES for c in XYZ_CASES)
assert len({c[0] for c in EDGE_CASES}) == len(EDGE_CASES) and len({c[0] for c in XYZ_CASES}) == len(XYZ_CASES)


def used_tiles(Cs, Cv):
    """32-column tiles of the 5 x 64 fused columns that hold features (q_tile_mask of svnet_edgeblock_wgrad_f32)."""
    used = 0
    for ct in range(10):
        if (Cs if ct < 4 else 2 * Cv) > 32 * (ct & 1):
            used |= 1 << ct
    return used


def split_tolerances(keys):
    """{key: bound}: outputs and running statistics at OUT_RTOL, gradients at GRAD_RTOL."""
    return {k: OUT_RTOL if k.startswith(("out", "buf:")) else GRAD_RTOL for k in keys}


# ----------------------------------------------------------------------------- inputs

def edge_inputs(case):
    """(params, s, v, rs, rv) of an edge-block case: H.module_params, every fourth linear1.beta column zero, scalars rounded to quarters,
    random upstream gradients."""
    tag, (Cs, Cv), (Os, Ov), B, N, k, _ = case
    params = H.module_params("SVBlock", ((2 * Cs, 2 * Cv), (Os, Ov), True), _stream(tag))
    params["linear1.beta"][:, ::4] = 0.0
    s, v = C.sv_pair(_stream(tag) + "/pt", (B, N), Cs, Cv, 1.0)
    s = torch.round(s * 4) / 4
    rs, rv = C.t(_stream(tag) + "/rs", (B, N, Os)), C.t(_stream(tag) + "/rv", (B, N, 3, Ov))
    return params, s, v, rs, rv


def xyz_inputs(case):
    """(params, x, rs, rv) of a first-layer case."""
    tag, nc, (Os, Ov), B, N, k, _ = case
    params = OrderedDict(("init_scalar." + n, t) for n, t in H.module_params("Vector2Scalar", (nc, 3, False, False), "envelope_xyz/%s/v2s" % tag).items())
    params.update(("conv1." + n, t) for n, t in H.module_params("SVBlock", ((3 * nc, nc), (Os, Ov), False), "envelope_xyz/%s/blk" % tag).items())
    x = C.small_cloud(B, N, 11 + nc)
    rs, rv = C.t("envelope_xyz/%s/rs" % tag, (B, N, Os)), C.t("envelope_xyz/%s/rv" % tag, (B, N, 3, Ov))
    return params, x, rs, rv


# ----------------------------------------------------------------------------- the oracle on a GIVEN graph, in any precision

def _cast(params, dtype, grad):
    return {n: (t.detach().to(dtype).clone().requires_grad_(grad and not n.endswith(("running_mean", "running_var"))) if t.is_floating_point() else t.clone())
            for n, t in params.items()}


def _buffers(P, ctx, prefix):
    return {"buf:" + n[len(prefix):]: ctx.bn_updates.get(n, t).detach().numpy() for n, t in P.items() if n.endswith(("running_mean", "running_var"))}


def edge_oracle(case, inputs, idx, dtype, train=True):
    """oracle.sv_ref (exact-STE train mode) on the graph `idx` [B,N,k] (cloud-local ids), in `dtype`: {out*, dx*, d:*, buf:*} as numpy
    (train) or {out*} (eval).  Only the oracle's k-NN insists on fp32; with the graph handed over everything runs in `dtype`."""
    tag, (Cs, Cv), (Os, Ov), B, N, k, _ = case
    params, s, v, rs, rv = inputs
    P = {"m." + n: t for n, t in _cast(params, dtype, train).items()}
    so, vo = s.detach().to(dtype).clone().requires_grad_(train), v.detach().to(dtype).clone().requires_grad_(train)
    ctx = sv_ref.Ctx(train=train, exact_ste=True, collect_bn=True)
    glob = (idx + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        oo, ov = sv_ref.svpool(sv_ref.svblock(sv_ref.graph_feature_sv((so, vo), k=k, idx=glob, ctx=ctx), P, "m", True, ctx), ctx=ctx)
    ref = {"out0": oo.detach().numpy(), "out1": ov.detach().numpy()}
    if not train:
        return ref
    ((oo * rs.to(dtype)).sum() + (ov * rv.to(dtype)).sum()).backward()
    ref.update({"dx0": so.grad.numpy(), "dx1": vo.grad.numpy()})
    ref.update({"d:" + n[2:]: t.grad.numpy() for n, t in P.items() if t.requires_grad})
    ref.update(_buffers(P, ctx, "m."))
    return ref


def edge_oracle_graph(case, inputs):
    """The oracle's own feature-space graph [B,N,k] of a case (fp32, exact)."""
    tag, (Cs, Cv), (Os, Ov), B, N, k, _ = case
    _, s, v, _, _ = inputs
    feat = torch.cat([s, v.reshape(B, N, -1)], dim=-1)
    return sv_ref.knn_indices(feat.transpose(-1, -2), k)


def xyz_oracle(case, inputs, idx, dtype, train=True):
    """get_graph_feature[_cross] -> Vector2Scalar -> SVBlock (fp) -> svpool of the oracle on the graph `idx` [B,N,k], in `dtype`."""
    tag, nc, (Os, Ov), B, N, k, _ = case
    params, x, rs, rv = inputs
    P = _cast(params, dtype, train)
    ctx = sv_ref.Ctx(train=train, collect_bn=True)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        ve = (sv_ref.graph_feature if nc == 2 else sv_ref.graph_feature_cross)(x.to(dtype).unsqueeze(1), k=k, idx=idx)
        s0 = sv_ref.vector2scalar(ve, P, "init_scalar")
        oo, ov = sv_ref.svpool(sv_ref.svblock((s0, ve), P, "conv1", False, ctx))
    ref = {"out0": oo.detach().numpy(), "out1": ov.detach().numpy()}
    if not train:
        return ref
    ((oo * rs.to(dtype)).sum() + (ov * rv.to(dtype)).sum()).backward()
    ref.update({"d:" + n: t.grad.numpy() for n, t in P.items() if t.requires_grad})
    ref.update(_buffers(P, ctx, ""))
    return ref


def quiet():
    return contextlib.redirect_stdout(io.StringIO())        # (the layer constructors print)
