"""CPU tests of the per-point attributes' host side: DevicePool's argument checks (svnet_amd/data.py), the argument checks of
svnet_batch_assemble_f32's attribute fields and of svnet_pool_gather_attr_f32 (nothing is launched), the ABI number, and the numpy
restatement the GPU tests compare against (tests/loader_attr_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

from tests import loader_attr_ref as RA
from tests import loader_ref as R

AUGS = {"none": (False, "none"), "scale_shift": (True, "none"), "z": (False, "z"), "so3": (False, "so3"), "scale_shift_so3": (True, "so3")}


def _arrays(M=5, P=32, A=6):
    rng = np.random.default_rng(3)
    return (rng.standard_normal((M, P, 3)).astype(np.float32), rng.integers(0, 40, M),
            rng.standard_normal((M, P, A)).astype(np.float32))


def test_pool_argument_checks_come_before_the_device_check():
    from svnet_amd.data import DevicePool
    data, label, attr = _arrays()
    bad = [(attr[0], 0, ValueError),                                        # rank
           (attr[:4], 0, ValueError), (attr[:, :8], 0, ValueError),         # M, P
           (attr[:, :, :0], 0, ValueError),                                 # A = 0
           (np.zeros((5, 32, 33), np.float32), 0, ValueError),              # A = 33
           (attr.astype(np.float64), 0, TypeError),
           (attr, 3, ValueError), (attr[:, :, :5], 2, ValueError),          # 3 k > A
           (attr, -1, ValueError),
           (None, 1, ValueError)]                                           # direction vectors of no attributes
    for a, k, err in bad:
        with pytest.raises(err, match="attr"):
            DevicePool(data, label, attr=a, attr_vectors=k, device="cpu")
    # well-formed arguments get as far as the device check
    for a, k in ((attr, 2), (attr, 0), (attr[:, :, :1], 0), (np.zeros((5, 32, 32), np.float32), 10)):
        with pytest.raises(RuntimeError):
            DevicePool(data, label, attr=a, attr_vectors=k, device="cpu")


def _desc(**over):
    """A descriptor whose pointers are non-null host addresses: only argument checks may look at it (nothing is launched)."""
    from svnet_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.BatchDesc()
    d._keep = buf
    d.data = d.label = d.seg = d.order = d.x = d.y = d.seg_out = d.onehot = d.params = d.attr = d.attr_out = p
    d.M, d.P, d.L, d.B, d.N, d.first, d.count, d.seed, d.epoch = 10, 2048, 10, 4, 1024, 0, 4, 1, 0
    d.select_mode, d.scale_shift, d.rotate, d.num_cat, d.A, d.attr_vectors = 0, 1, 0, 16, 6, 2
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over, word", [
    (dict(attr=None), b"attr_out without"),
    (dict(A=0), b"A 0 outside 1 .. 32"), (dict(A=33), b"A 33 outside 1 .. 32"), (dict(A=-1), b"A -1 outside"),
    (dict(attr_out=None, A=0), b"A 0 outside"),                       # a pool attr is checked even when nothing asks for it
    (dict(attr_vectors=3), b"attr_vectors 3"), (dict(A=5, attr_vectors=2), b"attr_vectors 2"), (dict(attr_vectors=-1), b"attr_vectors -1"),
    (dict(A=1, attr_vectors=1), b"attr_vectors 1"),
    (dict(N=4096), b"N 4096 > P 2048"),                               # (well-formed attributes: the other checks are still reached)
])
def test_attribute_argument_errors_return_minus_one_with_a_message(over, word):
    from svnet_amd import _lib
    L = _lib.lib()
    assert L.svnet_batch_assemble_f32(ctypes.byref(_desc(**over)), None) == -1
    assert word in L.svnet_last_error(), L.svnet_last_error()


def test_descriptor_ends_with_the_attribute_fields_and_zero_means_none():
    from svnet_amd import _lib
    names = [f[0] for f in _lib.BatchDesc._fields_]
    assert names[-4:] == ["attr", "A", "attr_vectors", "attr_out"] and names[-5] == "params"
    d = _lib.BatchDesc()
    assert d.attr is None and d.attr_out is None and d.A == 0 and d.attr_vectors == 0
    assert _lib.DEFINES["SVNET_BATCH_MAX_ATTR"] == 32
    # attributes take no LDS: svnet_batch_supported has the arguments it had
    assert len(_lib.SIGNATURES["svnet_batch_supported"][1]) == 3


def test_pool_gather_attr_argument_errors():
    from svnet_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args, word in (((None, p, 2, 8, 4, 3, p), b"null"), ((p, None, 2, 8, 4, 3, p), b"null"), ((p, p, 2, 8, 4, 3, None), b"null"),
                       ((p, p, 2, 8, 4, 0, p), b"A 0 outside 1 .. 32"), ((p, p, 2, 8, 4, 33, p), b"A 33 outside 1 .. 32"),
                       ((p, p, 0, 8, 4, 3, p), b"positive"), ((p, p, 2, 8, 0, 3, p), b"positive")):
        assert L.svnet_pool_gather_attr_f32(*args, None) == -1, args
        assert word in L.svnet_last_error(), L.svnet_last_error()
    assert L.svnet_pool_gather_attr_f32(p, p, 2, 1 << 40, 1 << 30, 3, p, None) == -2 and b"2^31" in L.svnet_last_error()


def test_header_binding_and_library_speak_abi_431():
    from svnet_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert _lib.lib().svnet_version() == _lib.ABI_VERSION >= 431
    assert "431: svnet_pool_gather_attr_f32, the attribute fields attr, A, attr_vectors, attr_out at the end of svnet_batch_desc" in header
    assert "svnet_pool_gather_attr_f32" in _lib.SIGNATURES and len(_lib.SIGNATURES["svnet_pool_gather_attr_f32"][1]) == 8
    assert os.path.basename(_lib.HEADER_PATH) == "svnet_hip.h"


# ----------------------------------------------------------------------------- the restatement itself (tests/loader_attr_ref.py)

def _pool(M=6, P=96, A=7, seed=5):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((M, P, 3)).astype(np.float32)
    attr = rng.standard_normal((M, P, A)).astype(np.float32)
    attr[:, :, 0:3] /= np.sqrt((attr[:, :, 0:3].astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)     # unit normals
    return data, rng.integers(0, 16, M), attr


@pytest.mark.parametrize("select", R.SELECT)
@pytest.mark.parametrize("aug", list(AUGS))
def test_scalar_channels_are_the_pools_by_exactly_the_restatements_perm(select, aug):
    scale_shift, rotate = AUGS[aug]
    data, label, attr = _pool()
    attr[2, 5, 4] = -0.0
    M, N = data.shape[0], 64
    order = R.epoch_order(9, 1, M)
    ref = R.batch(data, label, seed=9, epoch=1, first=0, count=M - 1, B=M, N=N, select=select, scale_shift=scale_shift, rotate=rotate,
                  order=order)
    params = np.zeros((M, 16), np.float32)
    params[:, 0:3], params[:, 3:6], params[:, 6:15] = ref["scale"], ref["shift"], ref["R"].reshape(M, 9).astype(np.float32)
    p32 = RA.points_fp32(attr, ref, params, 1, scale_shift, rotate)
    p64 = RA.points_f64(attr, ref, 1, scale_shift)
    assert p32.dtype == np.float32 and p32.shape == p64.shape == (M, 7, N)
    for b in range(M):
        want = attr[ref["m"][b]][ref["perm"][b]].T                               # [A,N]
        assert np.array_equal(p32[b, 3:].view(np.uint32), want[3:].view(np.uint32))
        assert np.array_equal(p64[b, 3:], want[3:].astype(np.float64))
        if aug == "none":
            assert np.array_equal(p32[b].view(np.uint32), want.view(np.uint32))  # direction groups too: the pool's bits
    assert np.array_equal(p32[M - 1], p32[0]) and not np.array_equal(p32[1], p32[0])   # the slot past count repeats slot 0


@pytest.mark.parametrize("aug", list(AUGS))
def test_the_rule_keeps_a_normal_perpendicular_to_its_surface_and_of_unit_length(aug):
    """The DEFINITION, in float64: points of a plane and the plane's unit normal go through the contract's transforms; the result is
    perpendicular to every transformed in-plane difference and has unit length, to 1e-12 relative.  (A rule that rotates but forgets
    the inverse scale fails the first with scale_shift on.)"""
    scale_shift, rotate = AUGS[aug]
    rng = np.random.default_rng(11)
    for g in range(8):
        ck = R.cloud_key(4, 2, g)
        scale, shift = R.scale_shift_of(ck) if scale_shift else (np.ones(3, np.float32), np.zeros(3, np.float32))
        Rm = R.rotation_of(ck, rotate)
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        u = np.cross(n, rng.standard_normal(3))
        v = np.cross(n, u)
        pts = rng.standard_normal(3) + rng.standard_normal((40, 1)) * u + rng.standard_normal((40, 1)) * v      # a planar patch
        assert abs((pts - pts[0]) @ n).max() < 1e-12
        moved = (pts * scale.astype(np.float64) + shift.astype(np.float64)) @ Rm.T                             # x' = R (S x + shift)
        out = RA.normal_f64(n, scale, Rm, scale_shift)
        diffs = moved[:, None, :] - moved[None, :, :]
        lengths = np.linalg.norm(diffs, axis=-1)
        assert abs(diffs @ out).max() <= 1e-12 * lengths.max(), (aug, g)
        assert abs(np.linalg.norm(out) - 1.0) <= 1e-12, (aug, g)
        if scale_shift:         # the rule that forgets the inverse scale is NOT perpendicular: the check above can tell them apart
            naive = Rm @ n
            assert abs(diffs @ naive).max() > 1e-3 * lengths.max()
    assert np.array_equal(RA.normal_f64(np.zeros(3), np.float32([0.7, 1.0, 1.4]), np.eye(3), True), np.zeros(3))        # zero stays zero


def test_fp32_evaluation_of_the_rule_is_within_the_derived_bound_of_float64():
    """FP32_BOUND is derived in tests/loader_attr_ref.py from the operation count (14 single-rounded operations on magnitudes <= 3/2,
    each within 2^-24 relative); both evaluations take the same scales and the fp32 rounding of the same R."""
    assert RA.FP32_BOUND == 14 * 1.5 * 2.0 ** -24
    data, label, attr = _pool(A=6)
    attr[:, :, 3:6] /= np.sqrt((attr[:, :, 3:6].astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
    attr[1, 7, 0:3] = 0.0                                                       # a zero vector is left as it is
    for aug, (scale_shift, rotate) in AUGS.items():
        ref = R.batch(data, label, seed=2, epoch=0, first=1, count=3, B=4, N=96, select="subset", scale_shift=scale_shift, rotate=rotate)
        params = np.zeros((4, 16), np.float32)
        params[:, 0:3], params[:, 3:6], params[:, 6:15] = ref["scale"], ref["shift"], ref["R"].reshape(4, 9).astype(np.float32)
        p32 = RA.points_fp32(attr, ref, params, 2, scale_shift, rotate)
        p64 = RA.points_f64(attr, ref, 2, scale_shift)
        err = float(abs(p32 - p64).max())
        print("%s: fp32 against float64 %.3e (bound %.3e)" % (aug, err, RA.FP32_BOUND))
        assert err <= RA.FP32_BOUND, (aug, err)
        if aug == "none":
            assert err == 0.0
        if scale_shift:
            lengths = np.sqrt((p32.astype(np.float64).reshape(4, 2, 3, 96) ** 2).sum(2))
            zero = (p32.reshape(4, 2, 3, 96) == 0).all(2)
            assert zero.sum() >= 1 and abs(lengths[~zero] - 1.0).max() < 4 * RA.FP32_BOUND      # unit length out
