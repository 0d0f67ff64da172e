"""The classifier's fused vector tail (csrc/vtail.hip, _ops.GlobalMaxMeanPoolBNV) at every edge of its dispatch, as ONE case table shared
by the GPU tests (tests/test_hip_kernel_tiers.py, section "vector tail": the kernels against float64) and the CPU tests
(tests/test_host_vtail_cases.py: the plan of every case against the library, the reference's own conditioning, the arg-max cap).

A case is (tag, B, N, C, expect) with expect = (CPL, planned chunks, chunks, rows per chunk, rows of the last chunk): the channels per
lane of the instantiation (C <= 64 -> 1, <= 128 -> 2, <= 192 -> 3) and what vtail_plan = split_plan(B, N, 768, 32, 8) of
csrc/split_reduce.h makes of the shape, restated below.  A workgroup's four waves take the rows r0 + w, r0 + w + 4, ... of a chunk two per
loop trip, so a last chunk of 1..7 rows is where a wave has no point at all (its key is the `any == false` zero) or only the first of its
two.  The scalar half's width stays at Ca = 5: it is GlobalMaxMeanPoolBN's pass, pinned by test_bn_pool_tiers.

The reference is not a reading of the kernel: it is the chain oracle/sv_ref.py:sv_dgcnn_cls runs behind conv5's products (svblock's
vector_bn * gate, svfuse's vector2scalar beside bn_act of the scalar half, max_over | mean over the points), composed here from the
oracle's own functions and run in float64 (the GPU tests' yard-stick) or float32 (its conditioning)."""
import functools

import numpy as np
import torch

from oracle import sv_ref

CA = 5                  # width of the scalar half in every case
SLOPE = 0.2             # conv5's LeakyReLU
OUT_RTOL = 1e-5         # tests/test_hip_kernel_tiers.py's bounds: outputs and running statistics ...
GRAD_RTOL = 1e-4        # ... and gradients, relative to the tensor's max (tests/common.py compare_case)
CONDITION = 0.25        # the float32 reference stays within this share of a bound on every case: the rest is the kernel's
REFERENCE_THREADS = 16  # how the float32 reference's row sums are split (conditioning() says why that has to be stated)


def _cdiv(a, b):
    return -(-a // b)


def split_plan(outer, R, target, least_rows, row_multiple=1):
    """csrc/split_reduce.h split_plan -> (planned chunks, chunks, rows per chunk)."""
    planned = max(1, min(_cdiv(target, outer), _cdiv(R, least_rows)))
    rows = _cdiv(_cdiv(R, planned), row_multiple) * row_multiple
    return planned, _cdiv(R, rows), rows


def vtail_plan(B, N):
    """csrc/vtail.hip vtail_plan: ~3 workgroups per CU, no chunk planned below 32 rows, rows a multiple of 8."""
    return split_plan(B, N, 256 * 3, 32, 8)


def cpl(C):
    return 1 if C <= 64 else (2 if C <= 128 else 3)


def plan_of(B, N, C):
    planned, chunks, rows = vtail_plan(B, N)
    return (cpl(C), planned, chunks, rows, N - (chunks - 1) * rows)


CASES = [
    ("c1_dead_lanes", 2, 256, 1, (1, 8, 8, 32, 32)),            # CPL 1 with 63 dead lanes; whole chunks
    ("c64_last_of_1", 3, 257, 64, (1, 9, 9, 32, 1)),            # CPL 1 full; waves 1..3 of the last chunk have no point
    ("c65_last_of_5", 2, 261, 65, (2, 9, 9, 32, 5)),            # one live lane in the second slot; wave 0's second point live, the others' dead
    ("c128_last_of_12", 2, 300, 128, (2, 10, 10, 32, 12)),      # CPL 2 full
    ("c129_last_of_3", 2, 259, 129, (3, 9, 9, 32, 3)),          # CPL 3 first; wave 3 of the last chunk idle
    ("c192_widest", 2, 512, 192, (3, 16, 16, 32, 32)),          # CPL 3 full, the widest admitted
    ("one_chunk", 768, 256, 3, (1, 1, 1, 256, 256)),            # one workgroup walks a whole cloud; 6912 outputs
    ("chunk_removed", 96, 257, 7, (1, 8, 7, 40, 17)),           # rounding the rows up to a multiple of 8 removes a chunk
    ("rows128", 100, 1000, 33, (1, 8, 8, 128, 104)),
]
BY_TAG = {c[0]: c for c in CASES}
KEYS = ("out", "dy", "dv", "dgate", "d:Wz", "d:scz", "d:gamma1", "d:beta1", "d:gamma2", "d:beta2",
        "buf:running_mean1", "buf:running_var1", "buf:running_mean2", "buf:running_var2")


def _gen(*key):
    """tests/test_hip_kernel_tiers.py _gen: seeded from the case's key, stable across runs and hosts."""
    s = 0
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(s)


def _signed(n, lo, hi, g):
    """n values of both signs with lo <= |.| <= hi."""
    mag = torch.rand(n, generator=g) * (hi - lo) + lo
    return torch.where(torch.arange(n) % 3 == 1, -mag, mag)


def inputs(case, variant=None):
    """float32 CPU tensors of one case: the two products conv5 leaves (y [B,N,Ca] before bn1, v [B,N,3,C] before VectorBN), the gate, both
    norms' parameters and running statistics, svfuse's Wz and scale, and an upstream gradient for the whole [B, 2 (Ca + 3C)] output.
    No zero vector and no planted tie, unless `variant` asks: "zeros" (a handful of points zeroed in some channels) or "ties" (one point
    in three rows of a cloud: both sides of the first chunk boundary and the one-row last chunk)."""
    tag, B, N, C, _ = case
    g = _gen("vtail", tag, B, N, C)
    d = {"y": torch.randn(B, N, CA, generator=g) * 2 + 0.3,
         "v": torch.randn(B, N, 3, C, generator=g) * (torch.rand(C, generator=g) + 0.2),
         "gate": torch.rand(B, C, generator=g) * 0.8 + 0.1,
         "gamma1": _signed(CA, 0.3, 1.5, g), "beta1": torch.randn(CA, generator=g) * 0.3,
         "rm1": torch.randn(CA, generator=g) * 0.3 + 0.3, "rv1": torch.rand(CA, generator=g) * 3 + 2,
         "gamma2": _signed(C, 0.3, 1.5, g), "beta2": _signed(C, 0.05, 0.4, g).flip(0),
         "rm2": torch.rand(C, generator=g) * 0.6 + 0.6, "rv2": torch.rand(C, generator=g) + 0.3,
         "Wz": torch.randn(3, C, generator=g), "scz": torch.rand(1, 3, generator=g) + 0.5,
         "gout": torch.randn(B, 2 * (CA + 3 * C), generator=g)}
    # The gradient of the [max] half is N(0.5, 1), of the [mean] half N(0, 1); both signs in each.  With a zero mean throughout, bn1's
    # dL/dbeta is a sum over the clouds that cancels, and at B * N = 24 672 rows the float32 REFERENCE's own row-by-row summation error
    # (3e-4 absolute) was 2.8e-5 of what was left; with 0.5 throughout, the [mean] half adds B * N small terms of one sign and the same
    # reference drifts by 3.7e-5 at B * N = 100 000.  Either is above a quarter of the bound without saying anything about a kernel.
    d["gout"][:, :CA + 3 * C] += 0.5
    d["Wz"][1, 0], d["Wz"][0, 0] = -1.7, 0.4                # outside and inside the STE window at every width
    if variant == "zeros":
        for b, r, c0 in ((0, 3, 0), (0, 31, 1), (1, 32, 0), (1, 256, 2), (1, N - 1, 64 % C)):
            d["v"][b, r, :, c0::7] = 0.0
    elif variant == "ties":
        first, again = TIE_ROWS[0], TIE_ROWS[1:]
        d["v"][:, first] *= TIE_SCALE
        for r in again:
            d["v"][:, r] = d["v"][:, first]
    else:
        assert variant is None
    return d


TIE_ROWS = (31, 32, 256)        # of c64_last_of_1: the last row of chunk 0, the first of chunk 1, the only row of chunk 8
TIE_SCALE = 4.0                 # the three copies together win many columns


def zero_vectors(v):
    """[B,N,3,C] bool: the entries of v's zero vectors."""
    return (v == 0).all(dim=2, keepdim=True).expand_as(v)


def reference(inp, dtype, train, pools=None, gate=True, binary=True):
    """The oracle's chain in `dtype` -> ({key: numpy}, info).  pools: an arg-max [B, Ca + 3C] to replay (oracle.sv_ref.Decisions, certified
    by info["dec"].check()); None = the run's own, returned as info["arg"].  info["f"] is the pooled feature [B,N,Ca+3C]."""
    t = {k: v.to(dtype) for k, v in inp.items()}
    B, N, C = t["v"].shape[0], t["v"].shape[1], t["v"].shape[-1]

    def leaf(x):
        return x.clone().requires_grad_(True)

    y, v = leaf(t["y"]), leaf(t["v"])
    gt = leaf(t["gate"]) if gate else None
    P = {"bn1.weight": leaf(t["gamma1"]), "bn1.bias": leaf(t["beta1"]), "bn1.running_mean": t["rm1"], "bn1.running_var": t["rv1"],
         "bn2.bn.weight": leaf(t["gamma2"]), "bn2.bn.bias": leaf(t["beta2"]), "bn2.bn.running_mean": t["rm2"], "bn2.bn.running_var": t["rv2"],
         "v2s.linear.weight": leaf(t["Wz"])}
    if binary:
        P["v2s.linear.scale"] = leaf(t["scz"])
    ctx = sv_ref.Ctx(train=train, collect_bn=True, exact_ste=True)
    if pools is not None:
        ctx.decisions = sv_ref.Decisions(pools=[pools.long()])
    else:
        ctx.decision_record = sv_ref.Decisions()
    u = sv_ref.vector_bn(v, P, "bn2", ctx)                                          # svblock: sv_layers.py:193-194
    if gt is not None:
        u = u * gt.view(B, 1, 1, C)
    s_v = sv_ref.vector2scalar(u, P, "v2s", binary=binary, ctx=ctx)                 # svfuse
    a = sv_ref.bn_act(y.reshape(-1, CA), P, "bn1", SLOPE, ctx).view(B, N, CA)       # svblock: sv_layers.py:188-190
    f = torch.cat([a, s_v], dim=-1)
    out = torch.cat((sv_ref.max_over(f, 1, ctx=ctx), f.mean(dim=1)), dim=1)         # sv_dgcnn_cls.py:69-74
    out.backward(t["gout"])

    def grad(p):
        return np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy()       # (eval: a bare sign(), no gradient reaches Wz)

    res = {"out": out.detach().numpy(), "dy": y.grad.numpy(), "dv": v.grad.numpy()}
    if gate:
        res["dgate"] = gt.grad.numpy()
    res["d:Wz"] = grad(P["v2s.linear.weight"])
    if binary:
        res["d:scz"] = grad(P["v2s.linear.scale"])
    for i, bn in ((1, "bn1"), (2, "bn2.bn")):
        res["d:gamma%d" % i], res["d:beta%d" % i] = grad(P[bn + ".weight"]), grad(P[bn + ".bias"])
        for stat in ("running_mean", "running_var"):
            new = ctx.bn_updates.get("%s.%s" % (bn, stat), P["%s.%s" % (bn, stat)]) if train else P["%s.%s" % (bn, stat)]
            res["buf:%s%d" % (stat, i)] = new.detach().numpy()
    info = {"dec": ctx.decisions, "f": f.detach(),
            "arg": (pools if pools is not None else ctx.decision_record.pools[0].reshape(B, -1)).long()}
    return res, info


def bounds(keys):
    return {k: OUT_RTOL if k.startswith(("out", "buf:")) else GRAD_RTOL for k in keys}


@functools.lru_cache(maxsize=None)
def conditioning(tag, train, variant=None, gate=True, binary=True):
    """(float32 run, float64 run on the float32 run's arg-max, the replay's Decisions, float64 pooled feature) of one case: computed once,
    shared by the CPU tests that read it, never changed."""
    inp = inputs(BY_TAG[tag], variant)
    # torch's float32 BatchNorm backward adds the rows of a thread's share one after the other, so the float32 run's dL/dbeta of bn1 depends
    # on the host's thread count: at 100 x 1000 rows (eval) it measured 2.3e-4, 8.5e-5, 4.4e-5, 3.0e-5, 2.3e-5, 1.0e-5 of the largest
    # element at 1, 2, 3, 4, 8, 16 threads - between twice the GPU bound and a tenth of it on the same inputs.  The split is pinned so
    # that the figure is the same number on every host; the float64 run, the GPU tests' only yard-stick, is at 1e-13 however it is split.
    threads = torch.get_num_threads()
    torch.set_num_threads(REFERENCE_THREADS)
    try:
        r32, i32 = reference(inp, torch.float32, train, gate=gate, binary=binary)
    finally:
        torch.set_num_threads(threads)
    r64, i64 = reference(inp, torch.float64, train, pools=i32["arg"], gate=gate, binary=binary)
    return r32, r64, i64["dec"], i32["arg"], i64["f"]


def split_dv(d, zero):
    """The two parts dv is compared in where the input holds zero vectors, each against its own largest element: there
    dL/dv = g * BN(n) / n * gate with n = EPS = 1e-6 is about 1e6 times an ordinary entry, and a bound relative to the whole tensor's
    largest element would leave the ordinary entries unchecked."""
    z = np.asarray(zero)
    return {"dv": d["dv"][~z]}, {"dv": d["dv"][z]}
