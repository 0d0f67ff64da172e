"""Times of the part-segmentation vector-neuron path on the GPU (svnet_amd/vn_pseg.py, csrc/vn_edge2.hip, csrc/vn_tail.hip) against the
module's own eval forward, by tools/time_vn.py's method: HIP events around repeated calls, legs alternating after a warm-up, the median
of the rounds with every round listed, eager and as captured graphs, everything in one process.  At the part-segmentation size:
B 32, N 2048, k 40 (--batch for a smaller B, which the report then names), seeded parameters and running statistics away from identity.
Each level's input is the level before's fused output, its neighbour list the k-NN of that input.

  (a) each of the three edge levels: the fused entry (tables and edge pass) against the module's eval forward on the same list,
      convs(get_graph_feature(x, idx=idx)).mean(-1);
  (b) the two-layer edge launch alone (svnet_vn_edge2_mean_f32 on tables that are already there), with the multiply-adds of its dense
      layer-2 product over its time as a fraction of the 155 TFLOP/s the f32-input MFMA sustains (the peak tools/time_sa_fused.py uses);
      the rest of the launch - layer 1's gather and both non-linearities - is vector work that the fraction does not count;
  (c) vn_std_coords alone, with the bytes it writes over its time;
  (d) the head in torch alone, as the wrapper runs it: the two products of conv8, bn8, the leaky rule, conv9 .. conv11;
  (e) FusedVNDGCNNPSeg(model)(x, l) against model(x, l), both with their dynamic graphs.

A ratio below 1 is marked LOSS.  Not measured here: hardware counters (where the gathered rows are served from, MFMA busy, LDS bank
conflicts of the two phases).

    python tools/time_vn_pseg.py [--out profiles/vn_pseg_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header
from time_vn import _worst
from time_vn_tail import _both

sys.path.insert(0, ROOT)

B, N, K = 32, 2048, 40
MFMA_F32_TFLOPS = 155.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--batch", type=int, default=B)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_vn_pseg.py measures on the GPU: no HIP device here")
    import numpy as np
    import svnet_amd.models as M
    from svnet_amd import _call, _lib, synth
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_pseg as VP
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.utils.vn_util import get_graph_feature, knn
    dev = torch.device("cuda:0")
    Bn = args.batch
    lines = [header(torch)]
    lines.append("B %d N %d k %d%s;  ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)"
                 % (Bn, N, K, "" if Bn == B else " (B %d asked for: the module path did not fit)" % B, args.inner, args.reps))
    torch.manual_seed(2024)
    model = M.VN_DGCNN_PSEG(argparse.Namespace(k=K, pooling="mean"), 50)
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            torch.nn.init.uniform_(m.weight, -1.5, 1.5)
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
            torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
            torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
    model = model.to(dev).eval()
    fused = VP.FusedVNDGCNNPSeg(model)
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, Bn, N))).to(dev)
    label = torch.from_numpy(np.ascontiguousarray(synth.category_onehot(7, 0, 0, Bn))).to(dev)
    assert fused.supported(Bn, N, K)
    reps, inner = args.reps, args.inner
    nograd = torch.no_grad()
    nograd.__enter__()

    # ---- (a) the levels, (b) the two-layer launch alone
    x, feats = cloud.view(Bn, 1, 3, N), []
    for i, ((convs, _), level) in enumerate(zip(model.edge_levels(), fused.levels)):
        idx = knn(x.view(Bn, -1, N), K)
        out = torch.empty(Bn, level[-1].O, 3, N, dtype=torch.float32, device=dev)
        two = len(level) == 2

        def leg_fused(x=x, idx=idx, level=level, out=out, two=two):
            return VF.vn_edge2_mean(x, idx, level[0], level[1], out=out) if two else VF.vn_edge_mean(x, idx, level[0], out=out)

        def leg_module(x=x, idx=idx, convs=convs):
            h = get_graph_feature(x, k=K, idx=idx)
            for conv in convs:
                h = conv(h)
            return h.mean(dim=-1)

        tag = "(a) level %d (C %d -> %s)" % (i + 1, level[0].C, " -> ".join(str(f.O) for f in level))
        labels = [("fused", "fused: tables + edge pass              "), ("module", "module: convs(get_graph_feature).mean  ")]
        _, _, last = _both(torch, dev, lines, tag, [("fused", leg_fused), ("module", leg_module)], labels, reps, inner, ratio=("module", "fused"))
        lines.append("%s  worst difference from the module relative to the largest value: %.2e" % (tag, _worst(last["fused"], last["module"])))
        if two:
            f1, f2 = level
            ws = f1.tables(Bn, N)
            alone = torch.empty_like(out)

            def leg_edge2(idx=idx, f1=f1, f2=f2, ws=ws, alone=alone):
                _lib.call("svnet_vn_edge2_mean_f32", _call.p(ws), ws.numel(), _call.p(idx), _call.p(f1.folded), _call.p(f2.folded), Bn, N, K, f1.C,
                          f1.O, f1.Od, f2.O, f2.Od, f1.slope, f2.slope, _call.p(alone), _call.stream())
                return alone

            tag = "(b) level %d" % (i + 1)
            eager, cap, _ = _both(torch, dev, lines, tag, [("edge2", leg_edge2)], [("edge2", "svnet_vn_edge2_mean_f32 alone          ")], reps, inner)
            flops = 2.0 * Bn * N * K * 3 * f1.O * (f2.O + f2.Od)
            for name, med in (("eager", eager), ("captured", cap)):
                if med:
                    lines.append("%s  %s: layer 2's product %.2f GFLOP in %.3f ms = %.2f TFLOP/s, %.1f %% of %g (layer 1 and the non-linearities not counted)"
                                 % (tag, name, flops / 1e9, med["edge2"], flops / med["edge2"] / 1e9, 100.0 * flops / med["edge2"] / 1e9 / MFMA_F32_TFLOPS,
                                    MFMA_F32_TFLOPS))
        x = leg_fused().clone()
        feats.append(x)
        del last
        torch.cuda.empty_cache()

    # ---- (c) the coordinates, (d) the head
    conv6, vn1, vn2 = fused.points
    w_lin = model.std_feature.vn_lin.weight.detach()
    x123 = torch.cat(feats, dim=1)
    local = VT.vn_point(x123, conv6)
    m = VT.vn_cloud_mean(local)
    y = VT.vn_point(VT.vn_point(local, vn1, cloud=m), vn2)
    pooled = VT.vn_std_pool(local, y, w_lin, cloud=m)[:, :6 * conv6.O].contiguous()
    e123 = VT.vn_std_coords(x123, y, w_lin)
    ebuf = torch.empty_like(e123)
    eager, cap, _ = _both(torch, dev, lines, "(c) coords", [("coords", lambda: VT.vn_std_coords(x123, y, w_lin, out=ebuf))],
                          [("coords", "vn_std_coords (63, 170)                ")], reps, inner)
    for name, med in (("eager", eager), ("captured", cap)):
        if med:
            lines.append("(c) coords  %s: %.1f MB written, %.1f MB read = %.2f TB/s" % (name, e123.numel() * 4 / 1e6, (x123.numel() + y.numel()) * 4 / 1e6,
                                                                                      (e123.numel() + x123.numel() + y.numel()) * 4 / med["coords"] / 1e9))
    w_const, w_point = fused._w8

    def head():
        const = torch.cat((pooled, model.conv7(label.view(Bn, -1, 1)).squeeze(-1)), dim=1) @ w_const.t()
        h8 = torch.matmul(w_point, e123).add_(const.unsqueeze(-1))
        for layer in list(model.conv8)[1:]:
            h8 = layer(h8)
        return model.head(h8)

    _both(torch, dev, lines, "(d) head", [("head", head)], [("head", "the head in torch, as the wrapper runs it")], reps, inner)
    del local, y, e123, ebuf, x123
    torch.cuda.empty_cache()

    # ---- (e) the model
    labels = [("fused", "FusedVNDGCNNPSeg(model)(x, l)          "), ("module", "model(x, l)                            ")]
    _both(torch, dev, lines, "(e) model", [("fused", lambda: fused(cloud, label)), ("module", lambda: model(cloud, label))], labels, reps, inner,
          ratio=("module", "fused"))
    got = fused(cloud, label)
    lines.append("(e) model  worst difference of the logits from the module on the same lists relative to the largest: %.2e"
                 % _worst(got, model(cloud, label, idx=fused.last_idx)))
    nograd.__exit__(None, None, None)
    emit(lines, args.out)


if __name__ == "__main__":
    main()
