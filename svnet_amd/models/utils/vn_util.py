"""Graph utilities of the vector-neuron models.

Drop-in for the reference module `models/utils/vn_util.py` (same names, arguments and defaults: knn :14, get_graph_feature :23,
get_graph_feature_cross :52).  Features are channel-first [B, C, 3, N]; a given `idx` [B, N, k] holds cloud-local ids, as in the
reference.  With `idx` given everything is plain torch and runs on any device; the dynamic graph is the library's k-NN kernel and
needs a HIP device.
"""
import torch

from ... import _ops

__all__ = ["knn", "get_graph_feature", "get_graph_feature_cross"]


def knn(x, k):
    """x: [B, C, N] -> [B, N, k] int64 neighbour ids (cloud-local, nearest first).  The reference's formula here is the one of
    sv_util.knn, which the kernel reproduces bit for bit (ties: lowest id first)."""
    return _ops.knn(x.detach(), k)


def _neighbours(x, k, idx, x_coord):
    """x [B, C, 3, N] -> (the neighbours' vectors, the centre's own repeated), both [B, C, 3, N, k]."""
    B, N = x.size(0), x.size(3)
    flat = x.reshape(B, -1, N)
    if idx is None:
        idx = knn(flat if x_coord is None else x_coord.reshape(B, -1, N), k=k)
    k = idx.size(-1)
    nb = torch.gather(flat, 2, idx.reshape(B, 1, N * k).expand(B, flat.size(1), N * k)).view(B, -1, 3, N, k)
    return nb, x.reshape(B, -1, 3, N, 1).expand_as(nb)


def get_graph_feature(x, k=20, idx=None, x_coord=None):
    """x: [B, C, 3, N] -> [B, 2C, 3, N, k]: channels [x_j - x_i | x_i] on the k-NN graph of x (of x_coord, or the given idx)."""
    nb, ctr = _neighbours(x, k, idx, x_coord)
    return torch.cat((nb - ctr, ctr), dim=1).contiguous()


def get_graph_feature_cross(x, k=20, idx=None):
    """x: [B, C, 3, N] -> [B, 3C, 3, N, k]: channels [x_j - x_i | x_i | x_j x x_i]."""
    nb, ctr = _neighbours(x, k, idx, None)
    return torch.cat((nb - ctr, ctr, torch.cross(nb, ctr, dim=2)), dim=1).contiguous()
