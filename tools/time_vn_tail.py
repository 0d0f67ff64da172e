"""Times of the fused vector-neuron tail on the GPU (svnet_amd/vn_tail.py, csrc/vn_tail.hip) against the module's own eval forward, by
tools/time_vn.py's method: HIP events around repeated calls, legs alternating after a warm-up, the median of the rounds with every
round listed, eager and as captured graphs.  At the classifier's size: B 32, N 1024, k 20, seeded parameters and running statistics
away from identity; the tail's inputs are the four fused levels' outputs.

  (a) the split of FusedVNDGCNN(model)(x) behind its fused levels, on the module path: the four k-NN calls each alone, conv5 (with the
      cat of the feats in front of it measured apart), the mean and the cat that build `both`, std_feature, the pools, the head;
  (b) each new entry alone into buffers allocated before the clock starts, with the multiply-adds its contract implies over its time;
  (c) FusedVNTail(model)(feats) against model.tail(feats) on the same inputs;
  (d) FusedVNDGCNN(model, tail=True)(x) against FusedVNDGCNN(model)(x).

A ratio below 1 is marked LOSS.  Not measured here: hardware counters (where the bytes are served from, MFMA busy), the cloud-term
launch apart from the point launch it precedes.

    python tools/time_vn_tail.py [--out profiles/vn_tail_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header
from time_vn import B, K, N, _captured, _report, _rounds, _verdict, _worst

sys.path.insert(0, ROOT)


def _both(torch, dev, lines, tag, legs, labels, reps, inner, ratio=None):
    """legs eager, then captured; ratio = (numerator key, denominator key) reported with a verdict."""
    res, med, last = _rounds(torch, legs, reps, inner)
    _report(lines, tag + "  eager   ", res, med, labels)
    if ratio:
        lines.append("%s  %s / %s, eager: %s" % (tag, ratio[0], ratio[1], _verdict(med[ratio[0]] / med[ratio[1]])))
    eager = med
    try:
        replays = [(k, _captured(torch, dev, fn)) for k, fn in legs]
    except Exception as e:                                      # a leg that cannot be captured: reported, not hidden
        lines.append("%s  captured graphs: not measured (%s: %s)" % (tag, type(e).__name__, str(e).splitlines()[0][:120]))
        return eager, None, last
    res, med, _ = _rounds(torch, [(k, r[0]) for k, r in replays], reps, inner)
    _report(lines, tag + "  captured", res, med, labels)
    if ratio:
        lines.append("%s  %s / %s, captured: %s" % (tag, ratio[0], ratio[1], _verdict(med[ratio[0]] / med[ratio[1]])))
    del replays
    torch.cuda.empty_cache()
    return eager, med, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_vn_tail.py measures on the GPU: no HIP device here")
    import numpy as np
    import torch.nn.functional as F
    import svnet_amd.models as M
    from svnet_amd import synth
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.utils.vn_util import knn
    dev = torch.device("cuda:0")
    lines = [header(torch)]
    lines.append("B %d N %d k %d;  ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)"
                 % (B, N, K, args.inner, args.reps))
    torch.manual_seed(2024)
    model = M.VN_DGCNN_CLS(argparse.Namespace(k=K, pooling="mean"), 40)
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            torch.nn.init.uniform_(m.weight, -1.5, 1.5)
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
            torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
            torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
    model = model.to(dev).eval()
    plain, fused = VF.FusedVNDGCNN(model), VF.FusedVNDGCNN(model, tail=True)
    tail = fused.tail
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, B, N))).to(dev)
    assert plain.supported(N, K) and tail.supported(B, N)
    reps, inner = args.reps, args.inner

    # the four levels' inputs and outputs, once
    h, inputs, feats = cloud.view(B, 1, 3, N), [], []
    for level in plain.levels:
        inputs.append(h)
        h = VF.vn_edge_mean(h, knn(h.view(B, -1, N), K), level).clone()
        feats.append(h)
    nograd = torch.no_grad()
    nograd.__enter__()

    # ---- (a) the split on the module path
    tag = "(a) module path"
    legs = [("knn%d" % (i + 1), (lambda x=x: knn(x.view(B, -1, N), K))) for i, x in enumerate(inputs)]
    labels = [("knn%d" % (i + 1), "k-NN of level %d, C %3d                 " % (i + 1, x.shape[1])) for i, x in enumerate(inputs)]
    x5 = torch.cat(feats, dim=1)
    local = model.conv5(x5)
    both = torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)
    inv = model.std_feature(both)[0]

    def pools(inv=inv):
        flat = inv.flatten(1, 2)
        return torch.cat((flat.amax(dim=-1), flat.mean(dim=-1)), dim=1)

    pooled = pools()

    def head(hh=pooled):
        for layer in (1, 2):
            linear, bn, drop = (getattr(model, "%s%d" % (n, layer)) for n in ("linear", "bn", "dp"))
            hh = drop(F.leaky_relu(bn(linear(hh)), negative_slope=0.2))
        return model.linear3(hh)

    legs += [("cat", lambda: torch.cat(feats, dim=1)), ("conv5", lambda: model.conv5(x5)),
             ("both", lambda: torch.cat((local, local.mean(dim=-1, keepdim=True).expand_as(local)), dim=1)),
             ("std", lambda: model.std_feature(both)[0]), ("pools", pools), ("head", head), ("tail", lambda: model.tail(feats))]
    labels += [("cat", "torch.cat of the four feats            "), ("conv5", "conv5                                  "),
               ("both", "the mean and the cat that build `both` "), ("std", "std_feature                            "),
               ("pools", "the [amax | mean] pools                "), ("head", "the head                               "),
               ("tail", "model.tail, all of the above           ")]
    eager, cap, _ = _both(torch, dev, lines, tag, legs, labels, reps, inner)
    for name, med in (("eager", eager), ("captured", cap)):
        if med:
            knn_ms = sum(med["knn%d" % i] for i in range(1, 5))
            lines.append("%s  %s: the four k-NN calls %.3f ms, model.tail %.3f ms (its parts add up to %.3f ms)"
                         % (tag, name, knn_ms, med["tail"], sum(med[k] for k in ("cat", "conv5", "both", "std", "pools", "head"))))
    del both, inv
    torch.cuda.empty_cache()

    # ---- (b) each new entry alone
    tag = "(b) entries"
    conv5, vn1, vn2 = tail.layers
    w_lin = model.std_feature.vn_lin.weight.detach()
    o5, m = VT.vn_point(x5, conv5), None
    m = VT.vn_cloud_mean(o5)
    o1 = VT.vn_point(o5, vn1, cloud=m)
    o2 = VT.vn_point(o1, vn2)
    hp = VT.vn_std_pool(o5, o2, w_lin, cloud=m, workspace=tail._std_ws)
    bufs = dict(o5=torch.empty_like(o5), m=torch.empty_like(m), o1=torch.empty_like(o1), o2=torch.empty_like(o2), hp=torch.empty_like(hp))
    legs = [("conv5", lambda: VT.vn_point(x5, conv5, out=bufs["o5"])), ("mean", lambda: VT.vn_cloud_mean(o5, out=bufs["m"])),
            ("vn1", lambda: VT.vn_point(o5, vn1, cloud=m, out=bufs["o1"])), ("vn2", lambda: VT.vn_point(o1, vn2, out=bufs["o2"])),
            ("std", lambda: VT.vn_std_pool(o5, o2, w_lin, cloud=m, out=bufs["hp"], workspace=tail._std_ws))]
    labels = [("conv5", "vn_point conv5 (169, 0, 341, 1)         "), ("mean", "vn_cloud_mean (341)                     "),
              ("vn1", "vn_point vn1 (341, 341, 341, 341) + term"), ("vn2", "vn_point vn2 (341, 0, 170, 170)         "),
              ("std", "vn_std_pool (341, 341, 170) + finish    ")]
    eager, cap, _ = _both(torch, dev, lines, tag, legs, labels, reps, inner)
    flop = {"conv5": 2.0 * B * N * 3 * 169 * 342, "vn1": 2.0 * B * N * 3 * 341 * 682 + 2.0 * B * 3 * 341 * 682, "vn2": 2.0 * B * N * 3 * 341 * 340,
            "std": 2.0 * B * N * (9 * 170 + 9 * 682)}
    for name, med in (("eager", eager), ("captured", cap)):
        if med:
            lines.append("%s  %s: " % (tag, name) + ";  ".join("%s %.2f GFLOP = %.1f TFLOP/s" % (k, f / 1e9, f / med[k] / 1e9) for k, f in flop.items())
                         + ";  mean: %.1f MB read = %.2f TB/s" % (o5.numel() * 4 / 1e6, o5.numel() * 4 / med["mean"] / 1e9))
    lines.append("%s  worst difference from the module path relative to the largest value: conv5 %.2e, pooled %.2e" % (tag, _worst(o5, local), _worst(hp, pooled)))
    del o1, o2, bufs, local
    torch.cuda.empty_cache()

    # ---- (c) the tail, (d) the model
    labels = [("fused", "FusedVNTail(model)(feats)              "), ("module", "model.tail(feats)                      ")]
    _, _, last = _both(torch, dev, lines, "(c) tail", [("fused", lambda: tail(feats)), ("module", lambda: model.tail(feats))], labels, reps, inner,
                       ratio=("module", "fused"))
    lines.append("(c) tail  worst difference of the logits from model.tail relative to the largest: %.2e" % _worst(tail(feats), model.tail(feats)))
    labels = [("tail", "FusedVNDGCNN(model, tail=True)(x)      "), ("plain", "FusedVNDGCNN(model)(x)                 ")]
    _both(torch, dev, lines, "(d) model", [("tail", lambda: fused(cloud)), ("plain", lambda: plain(cloud))], labels, reps, inner, ratio=("plain", "tail"))
    got = fused(cloud)
    lines.append("(d) model  worst difference of the logits from the module on the same lists relative to the largest: %.2e"
                 % _worst(got, model(cloud, idx=fused.last_idx)))
    nograd.__exit__(None, None, None)
    emit(lines, args.out)


if __name__ == "__main__":
    main()
