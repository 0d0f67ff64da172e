"""Times of the vector-neuron PointNet path on the GPU (svnet_amd/vn_pointnet.py, csrc/vn_cross.hip, csrc/vn_tail.hip) against the
module's own eval forward, by tools/time_vn.py's method: HIP events around repeated calls, legs alternating after a warm-up, the median
of the rounds with every round listed, eager and as captured graphs, everything in one process.  At the classification size:
B 32, N 1024, k 20 (--batch for a smaller B, which the report then names), seeded parameters and running statistics away from identity.

  (a) the position level: vn_edge_cross_mean against the module's conv_pos(get_graph_feature_cross(x, idx=idx)).mean(-1) on the same
      list, with the (edge, channel) pairs per second of the fused launch;
  (b) vn_point_norm alone (conv3 + bn3, 42 -> 341) against bn3(conv3(x)), with the bytes it writes over its time;
  (c) every stage of the wrapper alone, on the inputs the stage before it left: the k-NN, conv1, the transform net's three point
      layers, its cloud mean, its fc layers in torch, conv2 with the cloud term, the cloud mean of local, vn1, vn2, the
      standardise-and-pool stage (whose mean half this model does not read) and the head in torch;
  (d) FusedVNPointNet(model)(x) against model(x), both with their dynamic graph.

A ratio below 1 is marked LOSS.  Not measured here: hardware counters (where the gathered points are served from, how busy the
vector units are in the position level's non-linearity).

    python tools/time_vn_pointnet.py [--out profiles/vn_pointnet_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header
from time_vn import _worst
from time_vn_tail import _both

sys.path.insert(0, ROOT)

B, N, K = 32, 1024, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batch", type=int, default=B)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_vn_pointnet.py measures on the GPU: no HIP device here")
    import numpy as np
    import svnet_amd.models as M
    from svnet_amd import synth
    from svnet_amd import vn_pointnet as VP
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross, knn
    dev = torch.device("cuda:0")
    Bn = args.batch
    lines = [header(torch)]
    lines.append("B %d N %d k %d%s;  ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)"
                 % (Bn, N, K, "" if Bn == B else " (B %d asked for)" % B, args.inner, args.reps))
    torch.manual_seed(2024)
    model = M.VN_PointNet_CLS(argparse.Namespace(k=K, pooling="mean"), 40)
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            torch.nn.init.uniform_(m.weight, -1.5, 1.5)
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
            torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
            torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
    model = model.to(dev).eval()
    enc = model.feat
    fused = VP.FusedVNPointNet(model)
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, Bn, N))).to(dev)
    assert fused.supported(Bn, N, K)
    reps, inner = args.reps, args.inner
    P = fused.points
    nograd = torch.no_grad()
    nograd.__enter__()

    # ---- (a) the position level
    x4 = cloud.view(Bn, 1, 3, N)
    idx = knn(cloud, K)
    pos = torch.empty(Bn, fused.cross.O, 3, N, dtype=torch.float32, device=dev)
    legs = [("fused", lambda: VP.vn_edge_cross_mean(x4, idx, fused.cross, out=pos)),
            ("module", lambda: enc.conv_pos(get_graph_feature_cross(x4, k=K, idx=idx)).mean(dim=-1))]
    labels = [("fused", "fused: vn_edge_cross_mean              "), ("module", "module: conv_pos(graph_feature_cross).mean")]
    tag = "(a) position level (3 -> %d)" % fused.cross.O
    eager, cap, last = _both(torch, dev, lines, tag, legs, labels, reps, inner, ratio=("module", "fused"))
    lines.append("%s  worst difference from the module relative to the largest value: %.2e" % (tag, _worst(last["fused"], last["module"])))
    pairs = float(Bn) * N * K * fused.cross.O
    for name, med in (("eager", eager), ("captured", cap)):
        if med:
            lines.append("%s  %s: %.1f M (edge, channel) pairs in %.3f ms = %.1f G pairs/s" % (tag, name, pairs / 1e6, med["fused"], pairs / med["fused"] / 1e6))
    del last
    torch.cuda.empty_cache()

    # ---- the stages' inputs, by the wrapper's own path
    _, st = fused.encode(cloud, idx)
    x1, x2, local = st["conv1"], st["conv2"], st["local"]
    t1 = VT.vn_point(x1, P["fstn1"])
    t2 = VT.vn_point(t1, P["fstn2"])
    t3 = VT.vn_point(t2, P["fstn3"])
    tm = VT.vn_cloud_mean(t3)
    g = st["fstn"]
    m = VT.vn_cloud_mean(local)
    y1 = VT.vn_point(local, P["vn1"], cloud=m)
    y = VT.vn_point(y1, P["vn2"])
    w_lin = enc.std_feature.vn_lin.weight.detach()
    h = VT.vn_std_pool(local, y, w_lin, cloud=m)[:, :6 * fused.norm.O]

    # ---- (b) the norm-only layer
    nbuf = torch.empty_like(local)
    legs = [("fused", lambda: VT.vn_point_norm(x2, fused.norm, out=nbuf)), ("module", lambda: enc.bn3(enc.conv3(x2)))]
    labels = [("fused", "fused: vn_point_norm                   "), ("module", "module: bn3(conv3(x))                  ")]
    tag = "(b) conv3 + bn3 (%d -> %d)" % (fused.norm.C, fused.norm.O)
    eager, cap, last = _both(torch, dev, lines, tag, legs, labels, reps, inner, ratio=("module", "fused"))
    lines.append("%s  worst difference from the module relative to the largest value: %.2e" % (tag, _worst(last["fused"], last["module"])))
    for name, med in (("eager", eager), ("captured", cap)):
        if med:
            lines.append("%s  %s: %.1f MB written, %.1f MB read = %.2f TB/s" % (tag, name, local.numel() * 4 / 1e6, x2.numel() * 4 / 1e6,
                                                                              (local.numel() + x2.numel()) * 4 / med["fused"] / 1e9))
    del last, nbuf
    torch.cuda.empty_cache()

    # ---- (c) the stages of the wrapper, each alone
    bufs = {key: torch.empty_like(t) for key, t in (("conv1", x1), ("fstn1", t1), ("fstn2", t2), ("fstn3", t3), ("conv2", x2), ("vn1", y1), ("vn2", y))}
    stages = [("knn", "knn(x, %d)" % K, lambda: knn(cloud, K)),
              ("conv1", "vn_point conv1 (21 -> 21)", lambda: VT.vn_point(pos, P["conv1"], out=bufs["conv1"])),
              ("fstn1", "vn_point fstn.conv1 (21 -> 21)", lambda: VT.vn_point(x1, P["fstn1"], out=bufs["fstn1"])),
              ("fstn2", "vn_point fstn.conv2 (21 -> 42)", lambda: VT.vn_point(t1, P["fstn2"], out=bufs["fstn2"])),
              ("fstn3", "vn_point fstn.conv3 (42 -> 341)", lambda: VT.vn_point(t2, P["fstn3"], out=bufs["fstn3"])),
              ("fmean", "vn_cloud_mean of fstn.conv3", lambda: VT.vn_cloud_mean(t3)),
              ("ffc", "fstn.fc1 .. fc3 in torch", lambda: enc.fstn.head(tm)),
              ("conv2", "vn_point conv2 (21 + 21 cloud -> 42)", lambda: VT.vn_point(x1, P["conv2"], cloud=g, out=bufs["conv2"])),
              ("mean", "vn_cloud_mean of local", lambda: VT.vn_cloud_mean(local)),
              ("vn1", "vn_point vn1 (341 + 341 cloud -> 341)", lambda: VT.vn_point(local, P["vn1"], cloud=m, out=bufs["vn1"])),
              ("vn2", "vn_point vn2 (341 -> 170)", lambda: VT.vn_point(y1, P["vn2"], out=bufs["vn2"])),
              ("std", "vn_std_pool (341 + 341, 170)", lambda: VT.vn_std_pool(local, y, w_lin, cloud=m)),
              ("head", "the head in torch", lambda: model.head(h))]
    for key, label, fn in stages:
        _both(torch, dev, lines, "(c) stage", [(key, fn)], [(key, "%-40s" % label)], reps, inner)
    del bufs
    torch.cuda.empty_cache()

    # ---- (d) the model
    labels = [("fused", "FusedVNPointNet(model)(x)              "), ("module", "model(x)                               ")]
    _both(torch, dev, lines, "(d) model", [("fused", lambda: fused(cloud)), ("module", lambda: model(cloud))], labels, reps, inner, ratio=("module", "fused"))
    got = fused(cloud)
    lines.append("(d) model  worst difference of the logits from the module on the same list relative to the largest: %.2e"
                 % _worst(got, model(cloud, idx=fused.last_idx)))
    nograd.__exit__(None, None, None)
    emit(lines, args.out)


if __name__ == "__main__":
    main()
