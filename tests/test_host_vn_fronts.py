"""CPU tests of the order in which the vector-neuron front ends apply their checks (svnet_amd/_vn.py, vn_fused.py, vn_tail.py, vn_pseg.py,
vn_pointnet.py).  The `match=` tests of tests/test_host_vn*.py give every call one fault; here every call carries two, a pair of
consecutive links of the order stated in svnet_amd/_vn.py - the folded argument's type, the tensors (type, dtype, contiguity,
gradients), x's shape, idx's shape, the layer's input width, the other arguments' shapes, `out`, the HIP device - and the earlier
check's exception must win.  A wrapper's order: train mode, gradients, dtypes, x's shape, the other arguments, the neighbour lists,
their device, the HIP device.  No device is touched: the folded layers are tests/vn_cases.fake, the models have pooling = 'max'."""
import pytest
import torch

from tests import vn_cases as VC

B, N, k, C, Cg, O, O2, Cy = 2, 16, 4, 3, 2, 5, 6, 4
I64 = torch.int64
NO_CPU = (RuntimeError, "no CPU fallback")


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _edge_mean():
    from svnet_amd import vn_fused as VF
    x, idx, f, f4 = z(B, C, 3, N), z(B, N, k, dtype=I64), VC.fake(VF.FoldedVNLayer, C=C, O=O, Od=O), VC.fake(VF.FoldedVNLayer, C=4, O=O, Od=O)
    bad_out = z(B, O, N, 3)
    return VF.vn_edge_mean, [
        ("type, dtype", (x.double(), idx, object()), {}, TypeError, "folded must be a FoldedVNLayer"),
        ("tensor, dtype", (x.double(), idx.numpy(), f), {}, TypeError, "idx must be a tensor"),
        ("dtype, shape", (z(B, C, N).double(), idx, f), {}, TypeError, "x must be torch.float32"),
        ("dtype of out, shape", (z(B, C, N), idx, f), {"out": bad_out.double()}, TypeError, "out must be torch.float32"),
        ("contiguous, shape", (z(B, C, N, 3).transpose(2, 3), idx[:, :8].contiguous(), f), {}, ValueError, "x must be contiguous"),
        ("grad, shape", (z(B, C, N).requires_grad_(), idx, f), {}, ValueError, "x requires grad"),
        ("x, idx", (z(B, C, N), idx[:, :8].contiguous(), f), {}, ValueError, r"x must be \[B,C,3,N\]"),
        ("idx, width", (x, idx[:, :8].contiguous(), f4), {}, ValueError, r"idx must be \[B,N,k\]"),
        ("width, out", (x, idx, f4), {"out": bad_out}, ValueError, "the layer takes 4 vector channels"),
        ("out, device", (x, idx, f), {"out": bad_out}, ValueError, "out must be"),
        ("device, the layer's device", (x, idx, VC.fake(VF.FoldedVNLayer, C=C, O=O, Od=O, device=torch.device("meta"))), {}) + NO_CPU]


def _edge2_mean():
    from svnet_amd import vn_fused as VF
    from svnet_amd import vn_tail as VT
    x, idx = z(B, C, 3, N), z(B, N, k, dtype=I64)
    f1, f14 = VC.fake(VF.FoldedVNLayer, C=C, O=O, Od=O), VC.fake(VF.FoldedVNLayer, C=4, O=O, Od=O)
    f2, f2w = VC.fake(VT.FoldedVNPoint, C=O, Cg=0, O=O2, Od=O2), VC.fake(VT.FoldedVNPoint, C=O + 1, Cg=0, O=O2, Od=O2)
    bad_out = z(B, O, 3, N)
    return VF.vn_edge2_mean, [
        ("type 1, type 2", (x, idx, f2, f1), {}, TypeError, "folded1 must be a FoldedVNLayer"),
        ("type 2, dtype", (x.double(), idx, f1, f1), {}, TypeError, "folded2 must be a FoldedVNPoint"),
        ("dtype, shape", (z(B, C, N), idx.int(), f1, f2), {}, TypeError, "idx must be torch.int64"),
        ("grad, shape", (z(B, C, N).requires_grad_(), idx, f1, f2), {}, ValueError, "x requires grad"),
        ("x, idx", (z(B, C, N), idx[:, :8].contiguous(), f1, f2), {}, ValueError, r"x must be \[B,C,3,N\]"),
        ("idx, width", (x, idx[:, :8].contiguous(), f14, f2), {}, ValueError, r"idx must be \[B,N,k\]"),
        ("width 1, width 2", (x, idx, f14, f2w), {}, ValueError, "the first layer takes 4 vector channels"),
        ("width 2, out", (x, idx, f1, f2w), {"out": bad_out}, ValueError, "the second layer must take the first one's 5 channels"),
        ("out, device", (x, idx, f1, f2), {"out": bad_out}, ValueError, r"out must be \[B,O2,3,N\]"),
        ("device, the layers' device", (x, idx, f1, VC.fake(VT.FoldedVNPoint, C=O, Cg=0, O=O2, Od=O2, device=torch.device("meta"))), {}) + NO_CPU]


def _edge_cross_mean():
    from svnet_amd import vn_pointnet as VP
    x, idx, f = z(B, 1, 3, N), z(B, N, k, dtype=I64), VC.fake(VP.FoldedVNCross, O=O, Od=O)
    bad_out = z(B, O, N, 3)
    return VP.vn_edge_cross_mean, [
        ("type, dtype", (x.double(), idx, object()), {}, TypeError, "folded must be a FoldedVNCross"),
        ("dtype, shape", (z(B, 2, 3, N).double(), idx, f), {}, TypeError, "x must be torch.float32"),
        ("grad, shape", (z(B, 2, 3, N).requires_grad_(), idx, f), {}, ValueError, "x requires grad"),
        ("x, idx", (z(B, 2, 3, N), idx[:, :8].contiguous(), f), {}, ValueError, r"x must be \[B,1,3,N\]"),
        ("idx, out", (x, idx[:, :8].contiguous(), f), {"out": bad_out}, ValueError, r"idx must be \[B,N,k\]"),
        ("out, device", (x, idx, f), {"out": bad_out}, ValueError, "out must be"),
        ("device, the layer's device", (x, idx, VC.fake(VP.FoldedVNCross, O=O, Od=O, device=torch.device("meta"))), {}) + NO_CPU]


def _point():
    from svnet_amd import vn_tail as VT
    x, g = z(B, C, 3, N), z(B, Cg, 3)
    f, f4 = VC.fake(VT.FoldedVNPoint, C=C, Cg=Cg, O=O, Od=O), VC.fake(VT.FoldedVNPoint, C=4, Cg=Cg, O=O, Od=O)
    bad_out = z(B, O, N, 3)
    return VT.vn_point, [
        ("type, dtype", (x.double(), VC.fake(VT.FoldedVNPointNorm, C=C, O=O)), {}, TypeError, "folded must be a FoldedVNPoint "),
        ("tensor, dtype", (x.double(), f), {"cloud": g.numpy()}, TypeError, "cloud must be a tensor"),
        ("dtype, shape", (z(B, C, N), f), {"cloud": g.double()}, TypeError, "cloud must be torch.float32"),
        ("grad, shape", (z(B, C, N), f), {"cloud": g.clone().requires_grad_()}, ValueError, "cloud requires grad"),
        ("x, width", (z(B, C, N), f4), {"cloud": g}, ValueError, r"x must be \[B,C,3,N\]"),
        ("width, cloud", (x, f4), {}, ValueError, "the layer takes 4 vector channels per point"),
        ("cloud, out", (x, f), {"out": bad_out}, ValueError, r"cloud must be \[B,Cg,3\]"),
        ("out, device", (x, f), {"cloud": g, "out": bad_out}, ValueError, "out must be"),
        ("device, the layer's device", (x, VC.fake(VT.FoldedVNPoint, C=C, Cg=Cg, O=O, Od=O, device=torch.device("meta"))), {"cloud": g}) + NO_CPU]


def _point_norm():
    from svnet_amd import vn_tail as VT
    x, f, f4 = z(B, C, 3, N), VC.fake(VT.FoldedVNPointNorm, C=C, O=O), VC.fake(VT.FoldedVNPointNorm, C=4, O=O)
    bad_out = z(B, C, 3, N)
    return VT.vn_point_norm, [
        ("type, dtype", (x.double(), VC.fake(VT.FoldedVNPoint, C=C, Cg=0, O=O, Od=O)), {}, TypeError, "folded must be a FoldedVNPointNorm"),
        ("dtype, shape", (z(B, C, N).double(), f), {}, TypeError, "x must be torch.float32"),
        ("dtype of out, shape", (z(B, C, N), f), {"out": bad_out.double()}, TypeError, "out must be torch.float32"),
        ("x, width", (z(B, C, N), f4), {}, ValueError, r"x must be \[B,C,3,N\]"),
        ("width, out", (x, f4), {"out": bad_out}, ValueError, "the layer takes 4 vector channels per point"),
        ("out, device", (x, f), {"out": bad_out}, ValueError, "out must be"),
        ("device, the layer's device", (x, VC.fake(VT.FoldedVNPointNorm, C=C, O=O, device=torch.device("meta"))), {}) + NO_CPU]


def _cloud_mean():
    from svnet_amd import vn_tail as VT
    x = z(B, C, 3, N)
    return VT.vn_cloud_mean, [
        ("dtype, shape", (z(B, C, N).double(),), {}, TypeError, "x must be torch.float32"),
        ("grad, shape", (z(B, C, N).requires_grad_(),), {}, ValueError, "x requires grad"),
        ("x, out", (z(B, C, N),), {"out": z(B, C)}, ValueError, r"x must be \[B,C,3,N\]"),
        ("out, device", (x,), {"out": z(B, C)}, ValueError, r"out must be \[B,C,3\]")]


def _std_pool():
    from svnet_amd import vn_tail as VT
    x, y, w, g = z(B, C, 3, N), z(B, Cy, 3, N), z(3, Cy), z(B, Cg, 3)
    return VT.vn_std_pool, [
        ("dtype, shape", (z(B, C, N), y, w.double()), {}, TypeError, "w_lin must be torch.float32"),
        ("grad, shape", (z(B, C, N), y.clone().requires_grad_(), w), {}, ValueError, "y requires grad"),
        ("x, y", (z(B, C, N), z(B, Cy, 3, N + 1), w), {}, ValueError, r"x must be \[B,C,3,N\]"),
        ("y, w_lin", (x, z(B, Cy, 3, N + 1), z(2, Cy)), {}, ValueError, r"y must be \[B,Cy,3,N\]"),
        ("w_lin, cloud", (x, y, z(2, Cy)), {"cloud": z(B + 1, Cg, 3)}, ValueError, r"w_lin must be \[3,Cy\]"),
        ("cloud, out", (x, y, w), {"cloud": z(B + 1, Cg, 3), "out": z(B, 6 * C)}, ValueError, r"cloud must be \[B,Cg,3\] with B = 2"),
        ("out, device", (x, y, w), {"cloud": g, "out": z(B, 6 * C)}, ValueError, "out must be")]


def _std_coords():
    from svnet_amd import vn_tail as VT
    x, y, w = z(B, C, 3, N), z(B, Cy, 3, N), z(3, Cy)
    bad_out = z(B, C, 3, N)
    return VT.vn_std_coords, [
        ("dtype, shape", (z(B, C, N), y, w.double()), {}, TypeError, "w_lin must be torch.float32"),
        ("grad, shape", (z(B, C, N), y.clone().requires_grad_(), w), {}, ValueError, "y requires grad"),
        ("x, y", (z(B, C, N), z(B, Cy, 3, N + 1), w), {}, ValueError, r"x must be \[B,C,3,N\]"),
        ("y, w_lin", (x, z(B, Cy, 3, N + 1), z(2, Cy)), {}, ValueError, r"y must be \[B,Cy,3,N\]"),
        ("w_lin, out", (x, y, z(2, Cy)), {"out": bad_out}, ValueError, r"w_lin must be \[3,Cy\]"),
        ("out, device", (x, y, w), {"out": bad_out}, ValueError, r"out must be \[B,3C,N\]")]


ENTRIES = {"vn_edge_mean": _edge_mean, "vn_edge2_mean": _edge2_mean, "vn_edge_cross_mean": _edge_cross_mean, "vn_point": _point,
           "vn_point_norm": _point_norm, "vn_cloud_mean": _cloud_mean, "vn_std_pool": _std_pool, "vn_std_coords": _std_coords}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_raises_the_earlier_of_two_faults(entry):
    call, cases = ENTRIES[entry]()
    assert call.__name__ == entry
    for label, args, kw, exc, match in cases:
        with pytest.raises(exc, match=match) as info:
            call(*args, **kw)
        assert type(info.value) is exc and str(info.value).startswith(("%s: " % entry, "svnet_amd: ")), (label, info.value)


def _lists(n, meta=None, short=False):
    lists = [z(B, N, k, dtype=I64).to("meta" if i == meta else "cpu") for i in range(n)]
    return lists[:n - 1] if short else lists


def _dgcnn():
    from svnet_amd import vn_fused as VF
    x, flat = z(B, 3, N), z(B, N, 3)
    return VF.FusedVNDGCNN(VC.golden_model(None, "max")), (x,), [
        ("grad, dtype", (x.double().requires_grad_(),), {}, ValueError, "x requires grad"),
        ("dtype, shape", (flat.double(),), {}, TypeError, "x must be torch.float32"),
        ("x, lists", (flat,), {"idx": _lists(4, short=True)}, ValueError, r"x must be \[B,3,N\]"),
        ("lists, their device", (x,), {"idx": _lists(4, meta=1, short=True)}, ValueError, "four levels' neighbour lists"),
        ("lists' dtype, their device", (x,), {"idx": [i.int() for i in _lists(4, meta=1)]}, ValueError, "four levels' neighbour lists"),
        ("the lists' device, device", (x,), {"idx": _lists(4, meta=2)}, ValueError, r"x on cpu, idx\[2\] on meta"),
        ("device, the model's path", (x,), {"idx": _lists(4)}) + NO_CPU]


def _pseg():
    from svnet_amd import vn_pseg as VP
    from tests import vn_pseg_cases as PC
    x, flat, l = z(B, 3, N), z(B, N, 3), z(B, 16)
    return VP.FusedVNDGCNNPSeg(PC.golden_model(pooling="max")), (x, l), [
        ("grad of x, grad of l", (x.clone().requires_grad_(), l.clone().requires_grad_()), {}, ValueError, "x requires grad"),
        ("grad, dtype", (x.double(), l.clone().requires_grad_()), {}, ValueError, "l requires grad"),
        ("dtype, shape", (flat, l.double()), {}, TypeError, "l must be torch.float32"),
        ("x, l", (flat, z(B, 15)), {}, ValueError, r"x must be \[B,3,N\]"),
        ("l, lists", (x, z(B + 1, 16)), {"idx": _lists(3, short=True)}, ValueError, r"l must be \[B,16\] with B = 2"),
        ("lists, their device", (x, l), {"idx": _lists(3, meta=0, short=True)}, ValueError, "three levels' neighbour lists"),
        ("the lists' device, device", (x, l), {"idx": _lists(3, meta=2)}, ValueError, r"x on cpu, idx\[2\] on meta"),
        ("device, the model's path", (x, l), {"idx": _lists(3)}) + NO_CPU]


def _pointnet():
    from svnet_amd import vn_pointnet as VP
    from tests import vn_pointnet_cases as PC
    x, flat, idx = z(B, 3, N), z(B, N, 3), z(B, N, k, dtype=I64)
    return VP.FusedVNPointNet(PC.golden_model(pooling="max")), (x,), [
        ("grad, dtype", (x.double().requires_grad_(),), {}, ValueError, "x requires grad"),
        ("dtype, shape", (flat.double(),), {}, TypeError, "x must be torch.float32"),
        ("x, list", (flat,), {"idx": [idx]}, ValueError, r"x must be \[B,3,N\]"),
        ("list, its device", (x,), {"idx": idx.int().to("meta")}, ValueError, "the position level's neighbour list"),
        ("the list's device, device", (x,), {"idx": idx.to("meta")}, ValueError, "x on cpu, idx on meta"),
        ("device, the model's path", (x,), {"idx": idx}) + NO_CPU]


WRAPPERS = {"FusedVNDGCNN": _dgcnn, "FusedVNDGCNNPSeg": _pseg, "FusedVNPointNet": _pointnet}


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_wrapper_raises_the_earlier_of_two_faults(wrapper):
    fused, good, cases = WRAPPERS[wrapper]()
    assert type(fused).__name__ == wrapper and not fused.training
    fused.model.train()                                                           # train mode wins over everything that follows it
    for label, args, kw, exc, match in cases:
        with pytest.raises(RuntimeError, match="%s: the model is in train mode" % wrapper):
            fused(*args, **kw)
    fused.model.eval()
    for label, args, kw, exc, match in cases:
        with pytest.raises(exc, match=match) as info:
            fused(*args, **kw)
        assert type(info.value) is exc and str(info.value).startswith(("%s: " % wrapper, "svnet_amd: ")), (label, info.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # and a call with no fault but the device
        fused(*good)
