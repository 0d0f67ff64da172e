"""CPU tests of the extended k-NN range (4096 < N <= 32768, 64 < k <= 128): the contract itself and the C ABI's limits.

The first test pins the extension to the reference's own chain (dense matmul + topk on torch CPU, sv_util.py:19-25): the exact
oracle, which the GPU tests compare the kernel with, agrees with it there up to the order of exactly tied distances.  The others
need no GPU: the argument checks of the entry points return before any launch.
"""
import pytest
import torch

from oracle import knn as oknn
from svnet_amd import synth
from tests.golden import cases as C


@pytest.mark.parametrize("N,Cc,k,layout", [(6144, 62, 100, "nc"), (8192, 3, 20, "cn")])
def test_reference_chain_equals_exact_oracle_past_4096(N, Cc, k, layout):
    if layout == "cn":
        x = torch.from_numpy(synth.cloud_batch(C.SEED, 12, 0, 1, N))
    else:
        x = torch.from_numpy(synth.normal(C.SEED, synth.stream_id("host_knn_large/%d" % N), (1, N, Cc)) * 0.7).transpose(-1, -2)
    ref, pd = oknn.knn_exact(x, k, return_pd=True)
    got = oknn.knn_torch(x, k)
    assert oknn.tie_aware_mismatches(ref, got, pd) == 0


def _knn(L, B, N, Cc, k, ws_bytes=None):
    """svnet_knn_f32 on a fake device pointer: only the argument checks run (no launch happens before they pass)."""
    nbytes = L.svnet_knn_workspace_bytes(B, N, Cc) if ws_bytes is None else ws_bytes
    return L.svnet_knn_f32(16, B, N, Cc, N * Cc, 1, N, 1, k, 16, 16, nbytes, None)


def test_abi_refuses_past_the_extended_limits():
    from svnet_amd import _lib
    L = _lib.lib()
    E_UNSUPPORTED = _lib.DEFINES["SVNET_E_UNSUPPORTED"]
    assert _knn(L, 1, 32769, 3, 20) == E_UNSUPPORTED
    msg = L.svnet_last_error().decode()
    assert "32768" in msg and "128" in msg
    assert _knn(L, 1, 8192, 3, 129) == E_UNSUPPORTED
    assert "128" in L.svnet_last_error().decode()
    assert _knn(L, 1, 8192, 385, 20) == E_UNSUPPORTED
    assert "384" in L.svnet_last_error().decode()
    # the table path: k up to 128 at N <= 4096, nothing past
    assert L.svnet_knn_from_table_f32(16, 1 << 30, 1, 1024, 62, 129, 16, None) == E_UNSUPPORTED
    assert L.svnet_knn_from_table_f32(16, 1 << 30, 1, 8192, 62, 20, 16, None) == E_UNSUPPORTED
    assert L.svnet_knn_sv_f32(16, 20, 16, 3, 1, 32769, 20, 16, 16, 1 << 40, None) == E_UNSUPPORTED


def test_abi_accepts_the_extended_range_up_to_the_workspace_check():
    """Inside the new range the checks pass the size limits and stop at the workspace (given one byte too few): the range is open."""
    from svnet_amd import _lib
    L = _lib.lib()
    E_WORKSPACE = -3
    for B, N, Cc, k in [(8, 32768, 384, 128), (2, 4097, 3, 20), (1, 100, 7, 100), (2, 4096, 127, 65)]:
        need = L.svnet_knn_workspace_bytes(B, N, Cc)
        assert need >= (B * N * ((Cc + 7) // 8 * 8) + B * N) * 4
        assert _knn(L, B, N, Cc, k, need - 1) == E_WORKSPACE, (B, N, Cc, k, L.svnet_last_error())
    assert L.svnet_knn_from_table_f32(16, 1, 2, 1024, 62, 128, 16, None) == E_WORKSPACE
    # which forms the producers' table feeds is unchanged
    assert L.svnet_knn_table_fusable(2, 8192, 62) == 0 and L.svnet_knn_table_fusable(32, 1024, 62) == 1
