"""Times of the vector-neuron PointNet part-segmentation path on the GPU (svnet_amd/vn_pointnet_pseg.py; the wide envelope of
csrc/vn_tail.hip) against the module's own eval forward, by tools/time_vn_pseg.py's method: HIP events around repeated calls, legs
alternating after a warm-up, the median of the rounds with every round listed, eager and as captured graphs, everything in one process
on one neighbour list.  At the part-segmentation size: B 32, N 2048, k 40 (--batch for a smaller B, which the report then names),
seeded parameters and running statistics away from identity.  Each stage's input is the stage before's fused output.

  (a) every stage alone, the fused entries against the module's layers on the same input: the position level; conv1 .. conv3; the
      transform net; conv4 with its cloud channels; conv5 + bn5 (wide, norm only); the std tail (wide: mean, vn1, vn2, pool) against
      model.invariant and its maximum; both coordinate calls against the module's einsum on out1 .. out4; the head (below);
  (b) the wide launches alone - vn1 (682 + 682 -> 682 + 682 direction rows), vn2 (682 -> 341 + 341) and the norm-only 170 -> 682 - with
      the multiply-adds of their products over their time as a fraction of the 155 TFLOP/s the f32-input MFMA sustains (the peak
      tools/time_sa_fused.py uses), and the base envelope's vn1 of the siblings (341 + 341 -> 341 + 341) beside them;
  (c) the head's two variants: the mean's 2046 rows folded into G z (what the wrapper runs), and those rows existing per point - timed
      as the product over them alone on a tensor that is already there, a lower bound of any variant that writes them;
  (d) FusedVNPointNetPSeg(model)(x, l) against model(x, l), both with their dynamic graphs.

A ratio below 1 is marked LOSS.  Not measured here: hardware counters (MFMA busy, LDS bank conflicts, occupancy of the wide launches).

    python tools/time_vn_pointnet_pseg.py [--out profiles/vn_pointnet_pseg_times.txt]
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
        sys.exit("time_vn_pointnet_pseg.py measures on the GPU: no HIP device here")
    import numpy as np
    import svnet_amd.models as M
    from svnet_amd import synth
    from svnet_amd import vn_pointnet as VC
    from svnet_amd import vn_pointnet_pseg as VP
    from svnet_amd import vn_tail as VT
    from svnet_amd.models.utils.vn_util import get_graph_feature_cross, knn
    from svnet_amd.models.vn_layers import VNLinearLeakyReLU
    dev = torch.device("cuda:0")
    Bn = args.batch
    lines = [header(torch)]
    lines.append("B %d N %d k %d%s;  ms per call = HIP events around %d back-to-back calls; median of %d alternating rounds (all rounds listed)"
                 % (Bn, N, K, "" if Bn == B else " (B %d asked for: the module path did not fit)" % B, args.inner, args.reps))
    torch.manual_seed(2024)

    def seeded(module):
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                torch.nn.init.uniform_(m.weight, -1.5, 1.5)
                torch.nn.init.uniform_(m.bias, -0.5, 0.5)
                torch.nn.init.uniform_(m.running_mean, -0.25, 0.25)
                torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
        return module.to(dev).eval()

    model = seeded(M.VN_PointNet_PSEG(argparse.Namespace(k=K, pooling="mean"), 50))
    fused = VP.FusedVNPointNetPSeg(model)
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, Bn, N))).to(dev)
    label = torch.from_numpy(np.ascontiguousarray(synth.category_onehot(7, 0, 0, Bn))).to(dev)
    assert fused.supported(Bn, N, K)
    reps, inner = args.reps, args.inner
    nograd = torch.no_grad()
    nograd.__enter__()
    idx = knn(cloud, K)
    st = fused.encode(cloud, idx)
    P, w_lin = fused.points, model.std_feature.vn_lin.weight.detach()
    x4 = cloud.view(Bn, 1, 3, N)

    def stage(tag, fused_leg, module_leg, what):
        labels = [("fused", "fused: %-34s" % what[0]), ("module", "module: %-33s" % what[1])]
        _, _, last = _both(torch, dev, lines, tag, [("fused", fused_leg), ("module", module_leg)], labels, reps, inner, ratio=("module", "fused"))
        a, b = last["fused"], last["module"]
        lines.append("%s  worst difference from the module relative to the largest value: %.2e" % (tag, _worst(a, b)))
        del last
        torch.cuda.empty_cache()

    # ---- (a) the stages
    stage("(a) position level", lambda: VC.vn_edge_cross_mean(x4, idx, fused.cross),
          lambda: model.conv_pos(get_graph_feature_cross(x4, k=K, idx=idx)).mean(dim=-1), ("vn_edge_cross_mean", "conv_pos(graph feature).mean"))
    stage("(a) conv1 .. conv3", lambda: VT.vn_point(VT.vn_point(VT.vn_point(st["pos"], P["conv1"]), P["conv2"]), P["conv3"]),
          lambda: model.conv3(model.conv2(model.conv1(st["pos"]))), ("three vn_point", "conv3(conv2(conv1(pos)))"))

    def stn():
        t = st["out3"]
        for key in ("fstn1", "fstn2", "fstn3"):
            t = VT.vn_point(t, P[key])
        return model.fstn.head(VT.vn_cloud_mean(t))

    stage("(a) transform net", stn, lambda: model.fstn(st["out3"]), ("three vn_point, mean, fc in torch", "fstn(out3)"))
    g = st["fstn"]
    stage("(a) conv4, cloud = g", lambda: VT.vn_point(st["out3"], P["conv4"], cloud=g),
          lambda: model.conv4(torch.cat((st["out3"], g.unsqueeze(-1).expand(-1, -1, -1, N)), dim=1)), ("vn_point with 42 cloud channels", "conv4(cat(out3, g expanded))"))
    stage("(a) conv5 + bn5", lambda: VT.vn_point_norm(st["out4"], fused.norm), lambda: model.bn5(model.conv5(st["out4"])),
          ("wide vn_point_norm 170 -> 682", "bn5(conv5(out4))"))
    local = st["local"]

    def tail_module():
        out5, _ = model.invariant(st["out4"])
        return out5.max(dim=-1)[0]

    def tail_fused():
        return VT.std_tail(VT.vn_point_norm(st["out4"], fused.norm), P["vn1"], P["vn2"], w_lin, fused._std_ws, wide=True)[2][:, :6 * fused.norm.O]

    stage("(a) conv5 + bn5 + std tail", tail_fused, tail_module, ("wide norm, mean, vn1, vn2, pool", "invariant(out4), max over n"))
    skip_in = torch.cat((st["out1"], st["out2"], st["out3"], st["out4"]), dim=1)
    frame = torch.einsum("kc,bcan->bakn", w_lin, st["y"]).contiguous()

    def coords_fused():
        e = VT.vn_std_coords(torch.cat((st["out1"], st["out2"], st["out3"], st["out4"], fused._units(Bn, N, dev)), dim=1), st["y"], w_lin)
        return e[:, :skip_in.shape[1] * 3]

    stage("(a) e1234 (and the frame)", coords_fused,
          lambda: torch.einsum("bijm,bjkm->bikm", torch.cat((st["out1"], st["out2"], st["out3"], st["out4"]), dim=1), frame).reshape(Bn, -1, N),
          ("cat + vn_std_coords, 278 channels", "cat + einsum with a given frame"))
    stage("(a) e5", lambda: VT.vn_std_coords(local, st["y"], w_lin, wide=True), lambda: torch.einsum("bijm,bjkm->bikm", local, frame).reshape(Bn, -1, N),
          ("wide vn_std_coords, 682 channels", "einsum with a given frame"))
    del frame, skip_in
    torch.cuda.empty_cache()

    # ---- (b) the wide launches alone
    def rate(tag, key, leg, what, flops):
        eager, cap, _ = _both(torch, dev, lines, tag, [(key, leg)], [(key, what)], reps, inner)
        for name, med in (("eager", eager), ("captured", cap)):
            if med:
                lines.append("%s  %s: %.2f GFLOP in %.3f ms = %.2f TFLOP/s, %.1f %% of %g (the epilogue and, in eager, the cloud term's launch not counted)"
                             % (tag, name, flops / 1e9, med[key], flops / med[key] / 1e9, 100.0 * flops / med[key] / 1e9 / MFMA_F32_TFLOPS, MFMA_F32_TFLOPS))

    vn1, vn2 = P["vn1"], P["vn2"]
    m = st["m"]
    buf1 = torch.empty(Bn, vn1.O, 3, N, dtype=torch.float32, device=dev)
    rate("(b) wide vn1", "vn1", lambda: VT.vn_point(local, vn1, cloud=m, out=buf1), "vn_point 682 (+682 cloud) -> 682 + 682  ", 2.0 * Bn * N * 3 * vn1.C * (vn1.O + vn1.Od))
    buf2 = torch.empty(Bn, vn2.O, 3, N, dtype=torch.float32, device=dev)
    rate("(b) wide vn2", "vn2", lambda: VT.vn_point(buf1, vn2, out=buf2), "vn_point 682 -> 341 + 341               ", 2.0 * Bn * N * 3 * vn2.C * (vn2.O + vn2.Od))
    rate("(b) wide norm only", "norm", lambda: VT.vn_point_norm(st["out4"], fused.norm, out=local), "vn_point_norm 170 -> 682               ",
         2.0 * Bn * N * 3 * fused.norm.C * fused.norm.O)
    small = seeded(VNLinearLeakyReLU(682, 341, dim=4, negative_slope=0.0))
    f341 = VT.fold_vn_point(small, 341)
    x341, m341 = local[:, :341].contiguous(), m[:, :341].contiguous()
    buf3 = torch.empty(Bn, 341, 3, N, dtype=torch.float32, device=dev)
    rate("(b) base vn1 of the siblings", "vn1", lambda: VT.vn_point(x341, f341, cloud=m341, out=buf3), "vn_point 341 (+341 cloud) -> 341 + 341  ",
         2.0 * Bn * N * 3 * 341 * 682)
    del buf1, buf2, buf3, x341
    torch.cuda.empty_cache()

    # ---- (c) the head
    l2 = label
    whole = lambda: model.after_convs1(fused.convs1(st, l2))                      # noqa: E731
    _both(torch, dev, lines, "(c) head", [("head", whole)], [("head", "G z variant: convs1 by blocks, then the model's layers")], reps, inner)
    _both(torch, dev, lines, "(c) head", [("convs1", lambda: fused.convs1(st, l2))], [("convs1", "G z variant: convs1 by blocks alone               ")], reps, inner)
    w_mean = fused._w1[3].reshape(256, -1).contiguous()
    emean = torch.einsum("bia,bakn->bikn", m, torch.einsum("kc,bcan->bakn", w_lin, st["y"])).reshape(Bn, -1, N).contiguous()
    extra = torch.empty(Bn, 256, N, dtype=torch.float32, device=dev)
    _both(torch, dev, lines, "(c) head", [("rows", lambda: torch.matmul(w_mean, emean, out=extra))],
          [("rows", "per-point variant: the product over the mean's 2046 rows ALONE (they exist already)")], reps, inner)
    lines.append("(c) head  the per-point variant pays that product on top of everything the G z variant runs but its 9 rows, and the launch that writes "
                 "the rows (%.0f MB) besides" % (emean.numel() * 4 / 1e6))

    def module_head():
        out5, fr = model.invariant(st["out4"])
        pooled = torch.cat((out5.max(dim=-1)[0], l2), dim=1)
        e = torch.einsum("bijm,bjkm->bikm", torch.cat((st["out1"], st["out2"], st["out3"], st["out4"]), dim=1), fr).reshape(Bn, -1, N)
        return model.head(torch.cat((pooled.unsqueeze(-1).expand(-1, -1, N), e, out5), dim=1))

    got = whole()
    lines.append("(c) head  worst difference of the G z variant's logits from the module's behind out4, relative to the largest: %.2e" % _worst(got, module_head()))
    del emean, extra, got
    torch.cuda.empty_cache()

    # ---- (d) the model
    del st
    torch.cuda.empty_cache()
    labels = [("fused", "FusedVNPointNetPSeg(model)(x, l)       "), ("module", "model(x, l)                            ")]
    _both(torch, dev, lines, "(d) model", [("fused", lambda: fused(cloud, label)), ("module", lambda: model(cloud, label))], labels, reps, inner,
          ratio=("module", "fused"))
    got = fused(cloud, label)
    lines.append("(d) model  worst difference of the logits from the module on the same list relative to the largest: %.2e"
                 % _worst(got, model(cloud, label, idx=fused.last_idx)))
    nograd.__exit__(None, None, None)
    emit(lines, args.out)


if __name__ == "__main__":
    main()
