"""The contract of the fused binary chain (include/svnet_hip.h: svnet_bi_fold_f32, svnet_bi_chain_f32; svnet_amd/bi_fused.py) restated in
numpy, and the eval-mode forward of BiPointNet_CLS chained from it.  fl() is rounding to fp32; every operation is rounded once; nothing
is contracted but the stated fmaf (tests/sa_fused_ref.fmaf: one rounding); sgn(0) = 0.

    weight_sum(W)        the float64 sum of W in the fold kernel's order: lane t of 1024 adds W.flat[t], W.flat[t + 1024], .. in that order,
                         then the tree sh[i] += sh[i + s], s = 512 .. 1.
    fold_bi(W, scale, bn)  m = fl(S / (O K)); S = sgn(fl(W - m)); with BatchNorm (gamma, beta, mean, var, eps): invstd, s as
                         tests/sa_fused_ref.fold; a = fl(scale s), b = fl(beta - fl(mean s)); without: a = scale, b = +0.
    fold_fp(W, b, bn)    tests/sa_fused_ref.fold: (Wf, bf).
    chain(x, layers, trans, pool, offset, clamp)   per cloud: u = x, or u[n,j] = +0 then c ascending fmaf(x[c,n], T[c,j], u); an fp
                         layer t = bf then c ascending fmaf(u[c], Wf[o,c], t); a binary layer d = sum_c sgn(h[c]) S[o,c] (an exact integer),
                         t = fmaf(d, a, b); the next layer reads h = t.  write: t, clamped into [-1,1]; max: fl(max_n t + offset) - the
                         plain form; the kernel's integer extreme gives the same bits.
    bin_fc(h, f)         a fully connected binary layer on [B,K]: fmaf(d, a, b).
    forward(x, state)    FusedBiPointNet's seven steps -> the stages and, in `signs`, the sign of every BiLinearLSR input.

GOLDEN_CASE and synthetic_state are what tests/golden/make_bipointnet_golden.py records the reference on.
"""
import numpy as np

from svnet_amd import synth
from tests.sa_fused_ref import F32, F64, fmaf, fold as fold_fp_arrays, positive_zero      # noqa: F401  (positive_zero: re-exported)

GOLDEN_CASE = (11, 2, 1024, 40)                  # seed, B, N (in offset_map), num_class
OFFSET_MAP = {1024: -3.2041, 2048: -3.4025, 4096: -3.5836}
EPS = 1e-5
FOLD_LANES = 1024

# every BiLinearLSR of the classifier, in the order the forward reaches them
BI_POINT = ["feat.stn.conv2.lin", "feat.stn.conv3.lin", "feat.fstn.conv1.lin", "feat.fstn.conv2.lin", "feat.fstn.conv3.lin",
            "feat.conv2.lin", "feat.conv3.lin"]
BI_FC = ["feat.stn.fc1", "feat.stn.fc2", "feat.stn.fc3", "feat.fstn.fc1", "feat.fstn.fc2", "feat.fstn.fc3", "fc1", "fc2"]
BI_LAYERS = BI_POINT[:2] + BI_FC[:3] + BI_POINT[2:5] + BI_FC[3:6] + BI_POINT[5:] + BI_FC[6:]
CONTINUOUS = ["feat.stn.conv2.lin", "feat.fstn.conv1.lin", "feat.conv2.lin"]      # inputs that are not an affine of an integer count
STAGES = ["pool_stn", "trans", "pool_fstn", "trans_feat", "pool", "logits"]


def sgn(t):
    t = np.asarray(t)
    return (t > 0).astype(np.int8) - (t < 0).astype(np.int8)


def synthetic_state(keys, shapes, seed):
    """{key: array} for the state_dict layout `keys` / `shapes` (a scalar is ()).  Every draw is a function of (seed, key) alone.
    Linear weights ~ N(0, 1 / fan_in), biases 0.1 N; BiLinearLSR scales min(0.08, 1 / sqrt(fan_in)) U(0.9, 1) - inside 0.02 .. 0.08,
    so that scale * count has a standard deviation near 1; BatchNorm weights +-U(0.8, 1.6) with both signs, biases 0.2 N, running means
    0.25 N, running variances U(0.5, 1.5), num_batches_tracked 3."""
    out, keys = {}, [str(k) for k in keys]
    shape_of = {k: tuple(int(v) for v in s if int(v) >= 0) for k, s in zip(keys, shapes)}
    for key in keys:
        shape = shape_of[key]
        sid, leaf = synth.stream_id(key), key.rsplit(".", 1)[-1]
        stem = key[: -len(leaf)]
        norm = stem + "running_mean" in keys
        if leaf == "num_batches_tracked":
            out[key] = np.full((), 3, dtype=np.int64)
            continue
        if leaf == "scale":
            fan_in = shape_of[stem + "weight"][1]
            a = synth.uniform(seed, sid, (), 0.9, 1.0) * F32(min(0.08, 1.0 / np.sqrt(fan_in)))
            assert 0.02 <= float(a) <= 0.08
        elif leaf == "running_mean":
            a = synth.normal(seed, sid, shape) * F32(0.25)
        elif leaf == "running_var":
            a = synth.uniform(seed, sid, shape, 0.5, 1.5)
        elif leaf == "weight" and norm:
            a = synth.uniform(seed, sid, shape, 0.8, 1.6) * np.where(synth.integers(seed, sid, shape, 2) == 0, F32(1), F32(-1))
        elif leaf == "bias" and norm:
            a = synth.normal(seed, sid, shape) * F32(0.2)
        elif leaf == "weight":
            a = synth.normal(seed, sid, shape) / np.sqrt(F32(shape[1]))
        elif leaf == "bias":
            a = synth.normal(seed, sid, shape) * F32(0.1)
        else:
            raise KeyError(key)
        out[key] = np.array(a, dtype=F32).reshape(shape)
    return out


def golden_cloud():
    seed, B, N, _ = GOLDEN_CASE
    return synth.cloud_batch(seed, 0, 0, B, N)


# ---- the folds
def weight_sum(W):
    w = np.ascontiguousarray(W, dtype=F32).ravel().astype(F64)
    steps = -(-w.size // FOLD_LANES)
    w = np.concatenate([w, np.zeros(steps * FOLD_LANES - w.size)]).reshape(steps, FOLD_LANES)     # (adding +0.0 changes nothing)
    acc = np.zeros(FOLD_LANES)
    for row in w:
        acc = acc + row
    s = FOLD_LANES // 2
    while s > 0:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def fold_bi(W, scale, bn=None):
    """-> {"S": int8 [O,K], "a": [O], "b": [O], "m": float32}; bn = (gamma, beta, mean, var, eps) or None."""
    W = np.ascontiguousarray(W, dtype=F32)
    O = W.shape[0]
    m = F32(weight_sum(W) / F64(W.size))
    S = sgn((W - m).astype(F32))
    scale = F32(scale)
    if bn is None:
        a, b = np.full(O, scale, dtype=F32), np.zeros(O, dtype=F32)
    else:
        gamma, beta, mean, var = (np.ascontiguousarray(v, dtype=F32) for v in bn[:4])
        invstd = (F32(1) / np.sqrt((var + F32(bn[4])).astype(F32)).astype(F32)).astype(F32)
        s = (gamma * invstd).astype(F32)
        a = (scale * s).astype(F32)
        b = (beta - (mean * s).astype(F32)).astype(F32)
    return {"S": S, "a": a, "b": b, "m": m}


def fold_fp(W, b, bn):
    gamma, beta, mean, var, eps = bn
    return fold_fp_arrays(W, b, gamma, beta, mean, var, eps)[:2]


def _bn(state, prefix):
    return tuple(state[prefix + k] for k in ("weight", "bias", "running_mean", "running_var")) + (EPS,)


def fold_state_bi(state, lin, bn=None):
    return fold_bi(state[lin + ".weight"], state[lin + ".scale"], None if bn is None else _bn(state, bn + "."))


# ---- the chain
def counts(h, S):
    """d [rows, O]: the exact integer sum_c sgn(h[c]) S[o,c] (float64 products of small integers are exact)."""
    return sgn(h).astype(F64) @ S.astype(F64).T


def bin_fc(h, f, signs=None, key=None):
    if signs is not None:
        signs[key] = sgn(h)
    return fmaf(counts(h, f["S"]).astype(F32), f["a"], f["b"])


def chain_cloud(x, layers, trans=None, pool=None, offset=0.0, clamp=True, signs=None):
    """x [C0,N]; layers: ("fp", Wf, bf) - first only - or ("bi", folded[, key]) -> [O,N], or [O] with pool = "max".  With `signs`, the
    input sign of every keyed binary layer is stored there as [N,K] int8."""
    x = np.ascontiguousarray(x, dtype=F32)
    C0, N = x.shape
    if trans is None:
        u = np.ascontiguousarray(x.T)
    else:
        T = np.ascontiguousarray(trans, dtype=F32)
        u = np.zeros((N, C0), dtype=F32)
        for c in range(C0):
            u = fmaf(x[c][:, None], T[c][None, :], u)
    h = u
    for i, layer in enumerate(layers):
        if layer[0] == "fp":
            assert i == 0
            Wf, bf = layer[1], layer[2]
            t = np.broadcast_to(bf, (N, bf.shape[0])).astype(F32)
            for c in range(C0):
                t = fmaf(h[:, c][:, None], Wf[:, c][None, :], t)
        else:
            f = layer[1]
            if signs is not None and len(layer) > 2:
                signs[layer[2]] = sgn(h)
            t = fmaf(counts(h, f["S"]).astype(F32), f["a"], f["b"])
        h = t
    if pool == "max":
        return (h.max(axis=0) + F32(offset)).astype(F32)
    assert pool is None
    return np.ascontiguousarray((np.clip(h, F32(-1), F32(1)) if clamp else h).T)


def chain(x, layers, trans=None, pool=None, offset=0.0, clamp=True, signs=None):
    """x [B,C0,N] -> [B,O,N] or [B,O]; `signs` values become [B*N,K], rows ordered (b, n)."""
    per, outs = [], []
    for b in range(x.shape[0]):
        s = None if signs is None else {}
        outs.append(chain_cloud(x[b], layers, None if trans is None else trans[b], pool, offset, clamp, s))
        per.append(s)
    if signs is not None:
        for key in per[0]:
            signs[key] = np.concatenate([p[key] for p in per])
    return np.stack(outs)


# ---- the model
def tnet_head(pooled, state, prefix, k, signs):
    """The three fully connected layers of a transform net on the pooled [B,1024] and the identity -> [B,k,k]."""
    h = bin_fc(pooled, fold_state_bi(state, prefix + "fc1", prefix + "bn4"), signs, prefix + "fc1")
    h = bin_fc(h, fold_state_bi(state, prefix + "fc2", prefix + "bn5"), signs, prefix + "fc2")
    h = bin_fc(h, fold_state_bi(state, prefix + "fc3"), signs, prefix + "fc3")
    return (h + np.eye(k, dtype=F32).reshape(1, k * k)).astype(F32).reshape(-1, k, k)


def forward(x, state, offset=None):
    """The eval-mode forward of BiPointNet_CLS on x [B,3,N] -> ({stage: array}, {BiLinearLSR: its input's sign}); the logits, behind
    the last pooled tensor, are the head's fc3 in float64."""
    x = np.ascontiguousarray(x, dtype=F32)
    N = x.shape[2]
    off = OFFSET_MAP[N] if offset is None else offset
    signs, st = {}, {}

    def bi(key, bn):
        return ("bi", fold_state_bi(state, key, bn), key)

    def fp(conv, bn):
        return ("fp",) + tuple(fold_fp(state[conv + ".weight"], state[conv + ".bias"], _bn(state, bn + ".")))

    st["pool_stn"] = chain(x, [fp("feat.stn.conv1.lin", "feat.stn.bn1"), bi("feat.stn.conv2.lin", "feat.stn.bn2"),
                               bi("feat.stn.conv3.lin", "feat.stn.bn3")], pool="max", offset=off, signs=signs)
    st["trans"] = tnet_head(st["pool_stn"], state, "feat.stn.", 3, signs)
    st["h1"] = h1 = chain(x, [fp("feat.conv1.lin", "feat.bn1")], trans=st["trans"], clamp=True)
    st["pool_fstn"] = chain(h1, [bi("feat.fstn.conv1.lin", "feat.fstn.bn1"), bi("feat.fstn.conv2.lin", "feat.fstn.bn2"),
                                 bi("feat.fstn.conv3.lin", "feat.fstn.bn3")], pool="max", offset=off, signs=signs)
    st["trans_feat"] = tnet_head(st["pool_fstn"], state, "feat.fstn.", 64, signs)
    st["pool"] = chain(h1, [bi("feat.conv2.lin", "feat.bn2"), bi("feat.conv3.lin", "feat.bn3")], trans=st["trans_feat"], pool="max",
                       offset=off, signs=signs)
    h = bin_fc(st["pool"], fold_state_bi(state, "fc1", "bn1"), signs, "fc1")
    h = bin_fc(h, fold_state_bi(state, "fc2", "bn2"), signs, "fc2")
    st["fc2"] = h
    st["logits"] = np.clip(h, -1, 1).astype(F64) @ state["fc3.weight"].astype(F64).T + state["fc3.bias"].astype(F64)
    return st, signs


# ---- the recorded sign planes: ternary signs [rows,K] as two bit planes, > 0 and == 0
def pack_signs(s):
    return np.packbits(s > 0, axis=1), np.packbits(s == 0, axis=1)


def unpack_signs(pos, zero, K):
    p = np.unpackbits(pos, axis=1)[:, :K].astype(bool)
    z = np.unpackbits(zero, axis=1)[:, :K].astype(bool)
    return np.where(z, 0, np.where(p, 1, -1)).astype(np.int8)
