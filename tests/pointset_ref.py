"""What the numpy restatements of the point-set helpers share (tests/fps_ref.py, tests/propagate_ref.py, tests/group_ref.py): the
contract's distance, written from its statement in svnet_amd/csrc/pointset.h and independent of the kernels, and the lattice
coordinates on which it equals the reference's expanded form bit for bit.
"""
import numpy as np

from svnet_amd import synth

F32 = np.float32


def distances(a, b):
    """a [S,3], b [N,3] -> dist [S,N] float32 in the contract's order: d = fl(a - b) per coordinate, then
    fl(fl(fl(d0 d0) + fl(d1 d1)) + fl(d2 d2)) - every operation a single-rounded fp32 operation (numpy float32 arrays round each
    operation once and never fuse)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d0 = (a[:, None, 0] - b[None, :, 0]).astype(F32)
        d1 = (a[:, None, 1] - b[None, :, 1]).astype(F32)
        d2 = (a[:, None, 2] - b[None, :, 2]).astype(F32)
        return (((d0 * d0).astype(F32) + (d1 * d1).astype(F32)).astype(F32) + (d2 * d2).astype(F32)).astype(F32)


def lattice(seed, stream, shape):
    """Integer multiples of 2^-10 in [-1, 1): differences, squares and their sums are exact in fp32, so the reference's expanded
    distance form and the contract's difference form agree bit for bit, and every distance is a multiple of 2^-20."""
    return ((synth.integers(seed, stream, shape, 2048) - 1024).astype(np.float64) / 1024.0).astype(F32)
