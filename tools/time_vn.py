"""Times of the fused vector-neuron edge level on the GPU (svnet_amd/vn_fused.py, csrc/vn_edge.hip) against the module's own eval
forward, HIP events around repeated calls, at the classifier's size: B 32, N 1024, k 20, the four edge levels of VN_DGCNN_CLS,
(C, O) = (1, 21), (21, 21), (21, 42), (42, 85), with seeded parameters and running statistics away from identity.  Each level's input
is the level before's fused output, its neighbour list the k-NN of that input.  Per level, eager and as a captured graph:

  1. vn_edge_mean(x, idx, folded, out): the two launches behind the argument checks;
  2. layer(get_graph_feature(x, idx=idx)).mean(-1) in eval mode under no_grad: the module path - the yardstick, in the same process;
  3. svnet_vn_tables_f32 alone and svnet_vn_edge_mean_f32 alone, each into buffers allocated before the clock starts.

The edge pass's gather rate is the bytes the contract implies - per edge one neighbour row of 3 (O + Od) floats and one 8-byte id, per
point the centre's row and 3 O outputs - over its time; where those bytes are served from is not measured here.  Then the whole model,
FusedVNDGCNN(model)(x) against model(x), both with their dynamic graphs, eager and captured.

Legs alternate after a warm-up; the median of the rounds is reported with every round listed.  A ratio below 1 is marked LOSS.

    python tools/time_vn.py [--out profiles/vn_times.txt]
"""
import argparse
import sys

from event_timing import ROOT, emit, header, median, timed

sys.path.insert(0, ROOT)

B, N, K = 32, 1024, 20


def _rounds(torch, legs, reps, inner):
    for _, fn in legs:
        fn()
        fn()
    torch.cuda.synchronize()
    res, last = {k: [] for k, _ in legs}, {}
    for _ in range(reps):
        for k, fn in legs:
            t, last[k] = timed(torch, fn, inner)
            res[k].append(t)
    return res, {k: median(v) for k, v in res.items()}, last


def _verdict(ratio):
    return "%.2f x%s" % (ratio, "  LOSS" if ratio < 1.0 else "")


def _worst(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _captured(torch, dev, fn):
    """fn captured into a graph on a side stream after a warm-up there -> (replay, the graph)."""
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        res = fn()

    def replay():
        graph.replay()
        return res
    return replay, graph


def _report(lines, tag, res, med, labels):
    for k, label in labels:
        lines.append("%s  %s %9.3f ms  (%s)" % (tag, label, med[k], " ".join("%.3f" % v for v in res[k])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_vn.py measures on the GPU: no HIP device here")
    import numpy as np
    import svnet_amd.models as M
    from svnet_amd import synth
    from svnet_amd import vn_fused as VF
    from svnet_amd.models.utils.vn_util import get_graph_feature, knn
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
    fused = VF.FusedVNDGCNN(model)
    cloud = torch.from_numpy(np.ascontiguousarray(synth.cloud_batch(7, 0, 0, B, N))).to(dev)
    assert tuple(cloud.shape) == (B, 3, N) and fused.supported(N, K)

    x = cloud.view(B, 1, 3, N)
    for i, ((conv, _), folded) in enumerate(zip(model.edge_levels(), fused.levels)):
        C, O, Od = folded.C, folded.O, folded.Od
        idx = knn(x.view(B, -1, N), K)
        out = torch.empty(B, O, 3, N, dtype=torch.float32, device=dev)

        def leg_fused(x=x, idx=idx, folded=folded, out=out):
            return VF.vn_edge_mean(x, idx, folded, out=out)

        def leg_module(x=x, idx=idx, conv=conv):
            with torch.no_grad():
                return conv(get_graph_feature(x, k=K, idx=idx)).mean(dim=-1)

        def leg_tables(x=x, idx=idx, folded=folded, out=out):
            VF._launch(x, idx, folded, out, B, N, K, edge=False)
            return out

        def leg_edge(x=x, idx=idx, folded=folded, out=out):
            VF._launch(x, idx, folded, out, B, N, K, tables=False)
            return out

        tag = "level %d  C %d O %d" % (i + 1, C, O)
        res, med, last = _rounds(torch, [("fused", leg_fused), ("module", leg_module), ("tables", leg_tables), ("edge", leg_edge)], args.reps, args.inner)
        _report(lines, tag, res, med, (("fused", "vn_edge_mean, eager (2 launches)       "), ("module", "module eval forward, eager             "),
                                       ("tables", "svnet_vn_tables_f32 alone              "), ("edge", "svnet_vn_edge_mean_f32 alone           ")))
        row = 3 * (O + Od) * 4
        gather = B * N * K * (row + 8) + B * N * (row + 3 * O * 4)
        lines.append("%s  module / fused, eager: %s;  worst difference from the module relative to the largest output: %.2e"
                     % (tag, _verdict(med["module"] / med["fused"]), _worst(last["fused"], last["module"])))
        lines.append("%s  edge pass: %.1f MB implied by the contract (rows of %d B) in %.3f ms = %.2f TB/s;  tables: %.2f GFLOP in %.3f ms = %.1f TFLOP/s"
                     % (tag, gather / 1e6, row, med["edge"], gather / med["edge"] / 1e9, 2.0 * B * N * 3 * C * 2 * (O + Od) / 1e9, med["tables"],
                        2.0 * B * N * 3 * C * 2 * (O + Od) / med["tables"] / 1e9))
        try:
            replay_f, gf = _captured(torch, dev, leg_fused)
            replay_m, gm = _captured(torch, dev, leg_module)
            replay_t, gt = _captured(torch, dev, leg_tables)
            replay_e, ge = _captured(torch, dev, leg_edge)
        except Exception as e:                                  # a leg that cannot be captured: reported, not hidden
            lines.append("%s  captured graphs: not measured (%s: %s)" % (tag, type(e).__name__, str(e).splitlines()[0][:120]))
        else:
            res, med, last = _rounds(torch, [("fused", replay_f), ("module", replay_m), ("tables", replay_t), ("edge", replay_e)], args.reps, args.inner)
            _report(lines, tag, res, med, (("fused", "vn_edge_mean, captured graph           "), ("module", "module eval forward, captured graph    "),
                                           ("tables", "svnet_vn_tables_f32 alone, captured    "), ("edge", "svnet_vn_edge_mean_f32 alone, captured ")))
            lines.append("%s  module / fused, captured: %s" % (tag, _verdict(med["module"] / med["fused"])))
            del replay_f, replay_m, replay_t, replay_e, gf, gm, gt, ge
        x = VF.vn_edge_mean(x, idx, folded).clone()
        last.clear()
        torch.cuda.empty_cache()

    # ---- the whole model, dynamic graphs on both sides
    def leg_fused_model():
        return fused(cloud)

    def leg_model():
        with torch.no_grad():
            return model(cloud)

    tag = "VN_DGCNN_CLS"
    res, med, last = _rounds(torch, [("fused", leg_fused_model), ("module", leg_model)], args.reps, args.inner)
    _report(lines, tag, res, med, (("fused", "FusedVNDGCNN(model)(x), eager          "), ("module", "model(x) in eval mode, eager           ")))
    with torch.no_grad():
        replayed = model(cloud, idx=fused.last_idx)
    lines.append("%s  module / fused, eager: %s;  worst difference of the logits from the module on the same lists, relative to the largest: %.2e"
                 % (tag, _verdict(med["module"] / med["fused"]), _worst(fused(cloud), replayed)))
    try:
        replay_f, gf = _captured(torch, dev, leg_fused_model)
        replay_m, gm = _captured(torch, dev, leg_model)
    except Exception as e:
        lines.append("%s  captured graphs: not measured (%s: %s)" % (tag, type(e).__name__, str(e).splitlines()[0][:120]))
    else:
        res, med, last = _rounds(torch, [("fused", replay_f), ("module", replay_m)], args.reps, args.inner)
        _report(lines, tag, res, med, (("fused", "FusedVNDGCNN(model)(x), captured graph "), ("module", "model(x) in eval mode, captured graph  ")))
        lines.append("%s  module / fused, captured: %s" % (tag, _verdict(med["module"] / med["fused"])))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
