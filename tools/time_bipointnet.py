"""Times of the BiPointNet path on the GPU (svnet_amd/bi_fused.py, csrc/bi_chain.hip) against the module's own eval forward, by
tools/time_vn.py's method: HIP events around repeated calls, legs alternating after a warm-up, the median of the rounds with every round
listed, everything in one process.  At the classification size: B 32, N 1024 (--batch for a smaller B, which the report then names),
the seeded parameters of tests/bi_ref.synthetic_state.

  (a) the model: BiPointNet_CLS's eval forward, eager ONLY - BiLinearLSR.forward reads scale.item() on every call, a host read, so
      the module cannot be captured into a graph - against FusedBiPointNet(model)(x), eager and captured;
  (b) each chain launch alone, on the inputs the step before it left, with its implied int8 operation rate (2 K O per point and
      binary layer; the fp prefix is not counted);
  (c) the fully connected groups behind the maxima (three binary linear launches each) and the head;
  (d) the yardstick for fusion: chain D layer by layer on the entries the library already had - torch.bmm for the transform,
      svnet_binlinear_i8_fwd_f32 for conv2 and conv3 with the same folded a and b as scale and bias (it writes [B N, 1024] floats),
      svnet_bn_pool_fwd_f32 with identity statistics for the maximum - against the one fused launch.

A ratio below 1 is marked LOSS.  Not measured here: hardware counters (how busy the matrix cores are, LDS bank conflicts of the byte
stores), other cloud sizes, the part-segmentation widths.

    python tools/time_bipointnet.py [--out profiles/bipointnet_times.txt]
"""
import argparse
import sys
import types

from event_timing import ROOT, emit, header
from time_vn import _captured, _report, _rounds, _verdict, _worst
from time_vn_tail import _both

sys.path.insert(0, ROOT)

B, N = 32, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batch", type=int, default=B)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_bipointnet.py measures on the GPU: no HIP device here")
    import numpy as np
    import svnet_amd.models as M
    from svnet_amd import _call, _lib, synth
    from svnet_amd import bi_fused as BF
    from svnet_amd.models.bipointnet import offset_map
    from tests import bi_ref as R
    dev = torch.device("cuda:0")
    Bn, reps, inner = args.batch, args.reps, args.inner
    lines = [header(torch)]
    lines.append("B %d N %d%s;  ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)"
                 % (Bn, N, "" if Bn == B else " (B %d asked for)" % B, inner, reps))
    model = M.BiPointNet_CLS(types.SimpleNamespace(), 40)
    layout = model.state_dict()
    shapes = [list(v.shape) + [-1] * (2 - v.dim()) for v in layout.values()]
    state = R.synthetic_state(list(layout), shapes, 2024)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    model = model.to(dev).eval()
    fused = BF.FusedBiPointNet(model)
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, Bn, N))).to(dev)
    assert fused.supported(Bn, N)
    nograd = torch.no_grad()
    nograd.__enter__()

    # ---- (a) the model
    tag = "(a) model"
    res, med, last = _rounds(torch, [("fused", lambda: fused(cloud)[0]), ("module", lambda: model(cloud)[0])], reps, inner)
    _report(lines, tag + "  eager   ", res, med, (("fused", "FusedBiPointNet(model)(x)              "), ("module", "model(x) in eval mode                  ")))
    lines.append("%s  module / fused, eager: %s;  worst difference of the logits from the module relative to the largest: %.2e"
                 % (tag, _verdict(med["module"] / med["fused"]), _worst(last["fused"], last["module"])))
    lines.append("%s  the module is not captured: BiLinearLSR.forward reads scale.item() on every call, a host read" % tag)
    eager_module = med["module"]
    try:
        replay, graph = _captured(torch, dev, lambda: fused(cloud)[0])
        res, med, last2 = _rounds(torch, [("fused", replay)], reps, inner)
        _report(lines, tag + "  captured", res, med, (("fused", "FusedBiPointNet(model)(x)              "),))
        lines.append("%s  module eager / fused captured: %s;  the replay equals the eager result: %s"
                     % (tag, _verdict(eager_module / med["fused"]), bool(torch.equal(last2["fused"], last["fused"]))))
        del graph
    except Exception as e:                                              # reported, not hidden
        lines.append("%s  captured: not measured (%s: %s)" % (tag, type(e).__name__, str(e).splitlines()[0][:120]))

    # ---- (b) each chain launch alone
    st = fused.encode(cloud)
    C, off, ws = fused.chains, offset_map[N], fused._std_ws
    bufs = {k: torch.empty_like(st[k]) for k in ("pool_stn", "h1", "pool_fstn", "pool")}
    chains = [("A", "chain A: stn 3 -> 64 -> 128 -> 1024, max ", lambda: BF.bi_chain(cloud, C["A"], pool="max", offset=off, out=bufs["pool_stn"], workspace=ws)),
              ("B", "chain B: T 3x3, fp 3 -> 64, write        ", lambda: BF.bi_chain(cloud, C["B"], trans=st["trans"], out=bufs["h1"])),
              ("C", "chain C: fstn 64 -> 64 -> 128 -> 1024, max", lambda: BF.bi_chain(st["h1"], C["C"], pool="max", offset=off, out=bufs["pool_fstn"], workspace=ws)),
              ("D", "chain D: T 64x64, 64 -> 128 -> 1024, max  ", lambda: BF.bi_chain(st["h1"], C["D"], trans=st["trans_feat"], pool="max", offset=off, out=bufs["pool"], workspace=ws))]
    for key, label, fn in chains:
        eager, cap, _ = _both(torch, dev, lines, "(b) chain", [(key, fn)], [(key, label)], reps, inner)
        ops = 2.0 * Bn * N * sum(f.K * f.O for f in C[key] if isinstance(f, BF.FoldedBi))
        if ops:
            for name, m in (("eager", eager), ("captured", cap)):
                if m:
                    lines.append("(b) chain  %s %s: %.2f G int8 operations in %.3f ms = %.1f TOP/s" % (key, name, ops / 1e9, m[key], ops / m[key] / 1e9))

    # ---- (c) the fully connected groups
    groups = [("stn", "stn fc1 .. fc3 + identity (1024 -> 9)   ", lambda: fused._tnet(st["pool_stn"], "stn", 3)),
              ("fstn", "fstn fc1 .. fc3 + identity (1024 -> 4096)", lambda: fused._tnet(st["pool_fstn"], "fstn", 64)),
              ("head", "head fc1, fc2 binary, fc3 in torch      ", lambda: model.fc3(torch.clamp(fused.fcs["head"][1].linear_rows(fused.fcs["head"][0].linear_rows(st["pool"])), -1.0, 1.0)))]
    for key, label, fn in groups:
        _both(torch, dev, lines, "(c) fc   ", [(key, fn)], [(key, label)], reps, inner)

    # ---- (d) chain D layer by layer on the entries the library already had
    L = _lib.lib()
    conv2, conv3 = C["D"]
    packs = []
    for f in (conv2, conv3):
        w8 = torch.empty(int(L.svnet_binweight_i8_bytes(f.O, f.K)), dtype=torch.int8, device=dev)
        _lib.call("svnet_binweight_pack_i8", _call.p(f._s), f.O, f.K, _call.p(w8), _call.stream())
        packs.append(w8)
    M_rows = Bn * N
    y1 = torch.empty(M_rows, conv2.O, dtype=torch.float32, device=dev)
    y2 = torch.empty(M_rows, conv3.O, dtype=torch.float32, device=dev)
    O = conv3.O
    ident = {"mean": torch.zeros(O, device=dev), "invstd": torch.ones(O, device=dev), "gamma": torch.ones(O, device=dev), "beta": torch.zeros(O, device=dev)}
    nb = int(L.svnet_pool_workspace_bytes(Bn, N, O, 0)) + int(L.svnet_pool_workspace_bytes(Bn, N, O, 1))
    pws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    pmax, pmean = torch.empty(Bn, O, device=dev), torch.empty(Bn, O, device=dev)
    arg = torch.empty(Bn, O, dtype=torch.int32, device=dev)

    def layer(f, w8, src, dst):
        _lib.call("svnet_binlinear_i8_fwd_f32", _call.p(src), f.K, _call.p(f.zeros), _call.p(w8), _call.p(f.ab), _call.p(f.ab[f.O:]), M_rows, f.K, f.O,
                  _call.p(dst), None, None, None, None, _call.stream())

    def by_layer():
        u = torch.bmm(st["h1"].transpose(2, 1), st["trans_feat"]).reshape(M_rows, conv2.K)
        layer(conv2, packs[0], u, y1)
        layer(conv3, packs[1], y1, y2)
        _lib.call("svnet_bn_pool_fwd_f32", _call.p(y2), _call.p(ident["mean"]), _call.p(ident["invstd"]), _call.p(ident["gamma"]), _call.p(ident["beta"]),
                  Bn, N, O, 0, 0.0, _call.p(pmax), _call.p(pmean), O, _call.p(arg), _call.p(pws), nb, 0, _call.stream())
        return pmax + off

    tag = "(d) chain D"
    legs = [("fused", chains[3][2]), ("layers", by_layer)]
    labels = [("fused", "one launch: bi_chain                   "), ("layers", "bmm, binlinear_i8 x 2, bn_pool, + offset")]
    _, _, last = _both(torch, dev, lines, tag, legs, labels, reps, inner, ratio=("layers", "fused"))
    lines.append("%s  worst difference of the pooled tensor, layer by layer against fused, relative to the largest: %.2e (torch.bmm is not the "
                 "stated fmaf chain: a sign may flip)" % (tag, _worst(last["layers"], last["fused"])))
    lines.append("%s  the layer-by-layer form writes %.1f MB for conv3 alone; the fused launch writes %.3f MB" % (tag, y2.numel() * 4 / 1e6, Bn * O * 4 / 1e6))
    nograd.__exit__(None, None, None)
    emit(lines, args.out)


if __name__ == "__main__":
    main()
