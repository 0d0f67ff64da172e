"""Vector-neuron layers: the SO(3)-equivariant full-precision baseline of the SV models.

Drop-in for the reference module `models/vn_layers.py` (same class names, constructor arguments, defaults and state_dict keys, so a
reference checkpoint loads with strict=True): EPS :14, VNLinear :16, VNLeakyReLU :29, VNLinearLeakyReLU :50, VNBatchNorm :111,
VNMaxPool :134, mean_pool :151, VNStdFeature :155, STNkd :204.  Features are channel-first, [B, C, 3, N] or [B, C, 3, N, k]: C vector channels
of three components each.  Everything here is plain torch, train and eval, on any device; the fused eval-mode form of an edge
level (VNLinearLeakyReLU on an edge feature, then the mean over k) is svnet_amd/vn_fused.py.

Not here: VNLinearAndLeakyReLU (the reference's cannot be constructed: its __init__ names another class in super()).
"""
import torch
import torch.nn as nn

EPS = 1e-6

__all__ = ["EPS", "VNLinear", "VNLeakyReLU", "VNLinearLeakyReLU", "VNBatchNorm", "VNMaxPool", "mean_pool", "VNStdFeature", "STNkd"]


def _channels_last(linear, x):
    """A bias-free nn.Linear over the channel axis (axis 1) of x [B, C, 3, N, ...]."""
    return linear(x.transpose(1, -1)).transpose(1, -1)


def _leaky(p, d, negative_slope):
    """The vector-neuron leaky rule: where p points against the direction d, the component of p along d is taken out.
        y = slope p + (1 - slope) (p if <p,d> >= 0 else p - <p,d> / (|d|^2 + EPS) d)"""
    dotprod = (p * d).sum(2, keepdim=True)
    mask = (dotprod >= 0).to(p.dtype)
    d_norm_sq = (d * d).sum(2, keepdim=True)
    return negative_slope * p + (1 - negative_slope) * (mask * p + (1 - mask) * (p - (dotprod / (d_norm_sq + EPS)) * d))


class VNLinear(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.map_to_feat = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x):
        """x: [B, C, 3, N, ...] -> [B, O, 3, N, ...]"""
        return _channels_last(self.map_to_feat, x)


class VNLeakyReLU(nn.Module):
    def __init__(self, in_channels, share_nonlinearity=False, negative_slope=0.2):
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else in_channels, bias=False)
        self.negative_slope = negative_slope

    def forward(self, x):
        return _leaky(x, _channels_last(self.map_to_dir, x), self.negative_slope)


class VNBatchNorm(nn.Module):
    """BatchNorm on the vector norms: x / (|x| + EPS) * bn(|x| + EPS).  dim: the rank of x (3 or 4: BatchNorm1d, 5: BatchNorm2d)."""

    def __init__(self, num_features, dim):
        super().__init__()
        if dim not in (3, 4, 5):
            raise ValueError("VNBatchNorm: dim must be 3, 4 or 5 (the rank of the features), got %r" % (dim,))
        self.dim = dim
        self.bn = (nn.BatchNorm2d if dim == 5 else nn.BatchNorm1d)(num_features)      # the norms are [B, C, N] or [B, C, N, k]

    def forward(self, x):
        norm = torch.linalg.vector_norm(x, dim=2) + EPS
        norm_bn = self.bn(norm)
        return x / norm.unsqueeze(2) * norm_bn.unsqueeze(2)


class VNLinearLeakyReLU(nn.Module):
    """Linear, VNBatchNorm and the leaky rule with a learnt direction per output channel (share_nonlinearity: one for all)."""

    def __init__(self, in_channels, out_channels, dim=5, share_nonlinearity=False, negative_slope=0.2):
        super().__init__()
        self.dim = dim
        self.negative_slope = negative_slope
        self.map_to_feat = nn.Linear(in_channels, out_channels, bias=False)
        self.batchnorm = VNBatchNorm(out_channels, dim=dim)
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else out_channels, bias=False)

    def forward(self, x):
        p = self.batchnorm(_channels_last(self.map_to_feat, x))
        return _leaky(p, _channels_last(self.map_to_dir, x), self.negative_slope)


class VNMaxPool(nn.Module):
    """Over the last axis: per channel the vector with the largest projection on a learnt direction."""

    def __init__(self, in_channels):
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, in_channels, bias=False)

    def forward(self, x):
        d = _channels_last(self.map_to_dir, x)
        idx = (x * d).sum(2, keepdim=True).max(dim=-1, keepdim=False)[1]              # [B, C, 1, N, ...] without the last axis
        return torch.gather(x, -1, idx.expand(x.shape[:-1]).unsqueeze(-1)).squeeze(-1)


def _unit(v):
    """v [B, 3, ...] scaled to unit length along axis 1, EPS added to the length."""
    return v / (torch.sqrt((v * v).sum(1, keepdim=True)) + EPS)


def mean_pool(x, dim=-1, keepdim=False):
    return x.mean(dim=dim, keepdim=keepdim)


class VNStdFeature(nn.Module):
    """x [B, C, 3, N] -> (x expressed in a learnt equivariant frame z0 [B, 3, 3, N]: invariant features, z0)."""

    def __init__(self, in_channels, dim=4, normalize_frame=False, share_nonlinearity=False, negative_slope=0.2):
        super().__init__()
        self.dim = dim
        self.normalize_frame = normalize_frame
        half, quarter = in_channels // 2, in_channels // 4
        same = dict(dim=dim, share_nonlinearity=share_nonlinearity, negative_slope=negative_slope)
        self.vn1 = VNLinearLeakyReLU(in_channels, half, **same)
        self.vn2 = VNLinearLeakyReLU(half, quarter, **same)
        self.vn_lin = nn.Linear(quarter, 2 if normalize_frame else 3, bias=False)      # two rows: the third comes from the cross product

    def forward(self, x):
        rows = _channels_last(self.vn_lin, self.vn2(self.vn1(x)))                      # [B, 3 or 2, 3, N, ...]: the frame's vectors as rows
        if self.normalize_frame:                                                       # Gram-Schmidt on the two rows, the third their cross product
            first = _unit(rows[:, 0])
            second = rows[:, 1]
            second = _unit(second - (second * first).sum(1, keepdim=True) * first)
            rows = torch.stack((first, second, torch.cross(first, second, dim=1)), dim=1)
        frame = rows.transpose(1, 2)                                                   # [B, 3 components, 3 vectors, N, ...]
        # per point, every channel's vector in the frame's coordinates; the ellipsis stands for the N (, k) axes of any `dim`
        return torch.einsum('bij...,bjk...->bik...', x, frame), frame


class STNkd(nn.Module):
    """The transform net of the vector-neuron PointNet: x [B, d, 3, N] -> [B, d, 3], one equivariant vector per input channel.  Three
    point layers, the pool over the points, two layers on the pooled feature and a VNLinear; every leaky rule with slope 0."""

    def __init__(self, args, d=64):
        super().__init__()
        if args.pooling not in ("max", "mean"):
            raise ValueError("STNkd: pooling must be 'max' or 'mean', got %r" % (args.pooling,))
        self.args, self.d = args, d
        self.conv1 = VNLinearLeakyReLU(d, 64 // 3, dim=4, negative_slope=0.0)
        self.conv2 = VNLinearLeakyReLU(64 // 3, 128 // 3, dim=4, negative_slope=0.0)
        self.conv3 = VNLinearLeakyReLU(128 // 3, 1024 // 3, dim=4, negative_slope=0.0)
        self.fc1 = VNLinearLeakyReLU(1024 // 3, 512 // 3, dim=3, negative_slope=0.0)
        self.fc2 = VNLinearLeakyReLU(512 // 3, 256 // 3, dim=3, negative_slope=0.0)
        self.pool = VNMaxPool(1024 // 3) if args.pooling == "max" else mean_pool
        self.fc3 = VNLinear(256 // 3, d)

    def point_layers(self):
        """The three VNLinearLeakyReLU in front of the pool, in order."""
        return [self.conv1, self.conv2, self.conv3]

    def head(self, pooled):
        """What follows the pool: pooled [B, 341, 3] -> [B, d, 3]."""
        return self.fc3(self.fc2(self.fc1(pooled)))

    def forward(self, x):
        for conv in self.point_layers():
            x = conv(x)
        return self.head(self.pool(x))
