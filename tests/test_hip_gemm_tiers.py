"""GPU tests (-m gpu): every dispatch tier of svnet_gemm_f32 against a float64 product built on the CPU.

The case list is tests/gemm_cases.py (stated once; tests/test_host_gemm_cases.py checks the list and the comparison on the CPU).  Each
case builds its descriptor itself and calls svnet_gemm_f32 directly - not _ops.gemm, whose workspace policy keeps small M away from the
packed-B kernels - after asserting, on the real descriptor with the real device addresses, that svnet_gemm_tier / svnet_gemm_variant
name the family and variant the case is meant for.  C is pre-filled with a sentinel: the whole storage is compared, so padding between
rows (ldc > N) and the gaps a column stride leaves must keep it.  int cases are compared bit for bit, real cases per element with the
bound of gemm_cases.py; a failure names the case, family, variant and worst element.  Only valid descriptors are launched: refusals are
checked through the return code, with C untouched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _upload(c, x, dev):
    """Device tensors of a case's storage and {name: address} for gemm_cases.fill_desc."""
    t = {"B": _dev(x.B_store, dev), "C": _dev(x.C_store, dev)}
    if c["tern"]:
        t["a_sign"], t["a_nz"] = _dev(x.a_sign, dev), _dev(x.a_nz, dev)
    else:
        t["A"] = _dev(x.A_store, dev)
    if x.a_scale is not None:
        t["a_scale"] = _dev(x.a_scale_store, dev)
    for name in ("col_scale", "bias", "mask"):
        if getattr(x, name) is not None:
            t[name] = _dev(getattr(x, name), dev)
    if "col_sum" in c["epi"]:
        t["col_sum"] = torch.zeros((G.RED_SLICES + 1) * c["N"] + 2, dtype=torch.float32, device=dev)     # SVNET_SLICED_LEN(N)
    if c["ws"]:
        t["ws"] = torch.empty(G.workspace_bytes(c) + c["ws_off"] + 16, dtype=torch.uint8, device=dev)
    return t, {k: v.data_ptr() for k, v in t.items()}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c["name"] for c in G.RUN_CASES])
def test_gemm_case(c, kind, hip_device):
    from svnet_amd import _lib
    L = _lib.lib()
    x = G.build(c, kind)
    r = G.reference(c, x)
    t, ptr = _upload(c, x, hip_device)
    d = G.fill_desc(c, ptr, kind)
    got = (L.svnet_gemm_tier(ctypes.byref(d)), L.svnet_gemm_variant(ctypes.byref(d)))
    assert got == (c["tier"], c["variant"]), "%s: runs on %s variant %d, meant for %s variant %d" % (
        c["name"], G.FAMILY.get(got[0], got[0]), got[1], G.FAMILY[c["tier"]], c["variant"])
    _lib.call("svnet_gemm_f32", ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    C = t["C"].cpu().numpy()
    col = G.col_sum_of(t["col_sum"].cpu().numpy(), c["N"]) if "col_sum" in c["epi"] else None
    if kind == "real" and C.size and c["M"] and c["N"]:
        L_ = G.layout(c)
        worst, at, cw = G.ratios(c, x, r, G._view(C, 0, (c["M"], c["N"]), (L_["ldc"], L_["c_cs"])), col)
        print("%s real: worst element %.2f, column sums %.2f x 2^-24 of the bracket (bound %.1f)" % (c["name"], worst, cw, G.C_BOUND))
    bad = G.failures(c, x, r, C, col)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", G.REFUSALS, ids=[c["name"] for c in G.REFUSALS])
def test_refusal_launches_nothing(c, hip_device):
    from svnet_amd import _lib
    L = _lib.lib()
    x = G.build(c, "int")
    t, ptr = _upload(c, x, hip_device)
    d = G.fill_desc(c, ptr, "int")
    assert L.svnet_gemm_tier(ctypes.byref(d)) == c["rc"]
    assert L.svnet_gemm_f32(ctypes.byref(d), _stream()) == c["rc"]
    torch.cuda.synchronize()
    assert np.array_equal(t["C"].cpu().numpy(), x.C_store)
