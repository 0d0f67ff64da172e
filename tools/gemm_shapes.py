"""Which products of a workload's train step go through svnet_gemm_f32, on which path, and how long they take (diagnostic).
usage: python tools/gemm_shapes.py pointnet_fp|pointnet_bin|dgcnn_cls|partseg"""
import argparse, collections, contextlib, ctypes, io, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from svnet_amd import _lib, synth
from svnet_amd.train import cal_loss

wl = bench.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "pointnet_fp"]
dev = torch.device("cuda", 0)
import svnet_amd.models as M
from svnet_amd.train import seg_loss
torch.manual_seed(0)
cls, nc = {"sv_dgcnn_cls": (M.SV_DGCNN_CLS, 40), "sv_pointnet_cls": (M.SV_PointNet_CLS, 40), "sv_dgcnn_pseg": (M.SV_DGCNN_PSEG, 50)}[wl["model"]]
with contextlib.redirect_stdout(io.StringIO()):
    model = cls(argparse.Namespace(k=wl["k"], binary=wl["binary"], dropout=0.5), nc).to(dev).train()
B, N = wl["B"], wl["N"]
x = torch.from_numpy(synth.cloud_batch(1234, 0, 0, B, N)).to(dev)
if wl["model"] == "sv_dgcnn_pseg":
    inputs, y, loss_fn = (x, torch.from_numpy(synth.category_onehot(1234, 0, 0, B)).to(dev)), torch.from_numpy(synth.seg_labels(1234, 0, 0, B, N)).to(dev), seg_loss
else:
    inputs, y, loss_fn = (x,), torch.from_numpy(synth.class_labels(1234, 0, 0, B)).to(dev), cal_loss


TIER_NAMES = {v: k[len("SVNET_GEMM_"):].lower() for k, v in _lib.DEFINES.items() if k.startswith("SVNET_GEMM_")}


def path_of(d):
    """family/variant as the library's own queries name them (svnet_gemm_tier, svnet_gemm_variant: the dispatch is stated once)."""
    L = _lib.lib()
    return "%s/%d" % (TIER_NAMES.get(L.svnet_gemm_tier(ctypes.byref(d)), "refused"), L.svnet_gemm_variant(ctypes.byref(d)))


keys = []
def select(args):
    d = args[0]._obj
    keys.append((path_of(d), d.M, d.N, d.K, "A(rs=%d,cs=%d)" % (d.a_rs, d.a_cs), "B(rs=%d,cs=%d)" % (d.b_rs, d.b_cs), "exact" if d.b_exact else "fp32",
                 "".join(c for c, f in (("s", d.col_scale), ("b", d.bias), ("m", d.mask), ("c", d.col_sum), ("a", d.a_scale), ("+", d.accumulate)) if f)))
    return True


def step():
    for p in model.parameters():
        p.grad = None
    loss_fn(model(*inputs), y).backward()


step(); step()
torch.cuda.synchronize()
t = _lib.KernelTimer("svnet_gemm_f32", select)
_lib.TIMERS[:] = [t]
step()
torch.cuda.synchronize()
_lib.TIMERS[:] = []
tot, cnt = collections.Counter(), collections.Counter()
for k, ms in zip(keys, t.elapsed_ms()):
    tot[k] += ms; cnt[k] += 1
print("%d products, %.3f ms" % (len(keys), sum(tot.values())))
for k, ms in tot.most_common(60):
    print("%7.1f us x%-2d %s" % (ms * 1e3 / cnt[k], cnt[k], " ".join(str(x) for x in k)))
