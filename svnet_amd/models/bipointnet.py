"""The BiPointNet classification baseline (the reference's models/bipointnet.py, itself modified from github.com/htqin/BiPointNet): the
binary competitor that `sv_pointnet_cls --binary` is quoted against.  Plain torch, train and eval, any device; names, constructor
signatures, sub-module names and state_dict keys are the reference's, so its checkpoints load with strict=True, and the operations run
in its order, so the CPU results are its bits.

    offset_map          the 'ema-max' pooling's shift per cloud size: only 1024, 2048 and 4096 points have one, any other N raises
                        KeyError, as in the reference.
    Conv1d              a Linear over the channels of [B,C,N].
    BiSTN3d, BiSTNkd    the input and the feature transform nets: three shared layers, a pooling over the cloud, three fully connected
                        layers, plus the identity.
    BiPointNetEncoder   stn -> bmm -> conv1 -> fstn -> bmm -> conv2 -> conv3 -> pooling.
    BasicBiPointNet     the encoder and a three-layer head; forward returns (logits, trans_feat).
    BiPointNetLSREMax   BasicBiPointNet with BiLinearLSR layers and pool = 'ema-max': models.BiPointNet_CLS.

Not ported: the part-segmentation and the semantic-segmentation models.  svnet_amd.bi_fused.FusedBiPointNet is the fused eval forward.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .bipointnet_basic import BiLinearLSR

__all__ = ["offset_map", "Conv1d", "BiSTN3d", "BiSTNkd", "BiPointNetEncoder", "BasicBiPointNet", "BiPointNetLSREMax"]

offset_map = {
    1024: -3.2041,
    2048: -3.4025,
    4096: -3.5836,
}


class Conv1d(nn.Module):
    """`Linear(inplane, outplane)` applied to every point of [B,C,N] -> [B,outplane,N]."""

    def __init__(self, inplane, outplane, Linear):
        super().__init__()
        self.lin = Linear(inplane, outplane)

    def forward(self, x):
        B, C, N = x.shape
        rows = x.permute(0, 2, 1).contiguous().view(-1, C)
        return self.lin(rows).view(B, N, -1).permute(0, 2, 1).contiguous()


def _pool_tnet(x, bn3, conv3, pool, N):
    """The third shared layer of a transform net and its pooling -> [B,1024]."""
    if pool == "max":
        x = torch.max(F.hardtanh(bn3(conv3(x))), 2, keepdim=True)[0]
    elif pool == "mean":
        x = torch.mean(F.hardtanh(bn3(conv3(x))), 2, keepdim=True)
    elif pool == "ema-max":
        x = bn3(conv3(x)) + offset_map[N]
        x = torch.max(x, 2, keepdim=True)[0]
    return x.view(-1, 1024)


class _BiSTN(nn.Module):
    """What the two transform nets share: the layers behind conv1 and the forward.  `k`: the transform is [k,k]."""

    def _build(self, first, k, Linear, pool, affine):
        self.conv1 = first
        self.conv2 = Conv1d(64, 128, Linear)
        self.conv3 = Conv1d(128, 1024, Linear)
        self.fc1 = Linear(1024, 512)
        self.fc2 = Linear(512, 256)
        self.fc3 = Linear(256, k * k)
        self.bn1 = nn.BatchNorm1d(64, affine=affine)
        self.bn2 = nn.BatchNorm1d(128, affine=affine)
        self.bn3 = nn.BatchNorm1d(1024, affine=affine)
        self.bn4 = nn.BatchNorm1d(512, affine=affine)
        self.bn5 = nn.BatchNorm1d(256, affine=affine)
        self.pool = pool

    def point_part(self, x):
        """x [B,D,N] -> the pooled [B,1024]."""
        N = x.size(2)
        x = F.hardtanh(self.bn1(self.conv1(x)))
        x = F.hardtanh(self.bn2(self.conv2(x)))
        return _pool_tnet(x, self.bn3, self.conv3, self.pool, N)

    def head(self, x, k):
        """The pooled [B,1024] -> the transform [B,k,k]."""
        B = x.size(0)
        x = F.hardtanh(self.bn4(self.fc1(x)))
        x = F.hardtanh(self.bn5(self.fc2(x)))
        x = self.fc3(x)
        iden = torch.eye(k, device=x.device).view(1, k * k).repeat(B, 1)
        return (x + iden).view(-1, k, k)


class BiSTN3d(_BiSTN):
    def __init__(self, channel, Linear=BiLinearLSR, pool="max", affine=True, bi_first=False):
        super().__init__()
        self._build(Conv1d(channel, 64, Linear if bi_first else nn.Linear), 3, Linear, pool, affine)

    def forward(self, x):
        return self.head(self.point_part(x), 3)


class BiSTNkd(_BiSTN):
    def __init__(self, k=64, Linear=BiLinearLSR, pool="max", affine=True, bi_first=False):
        super().__init__()
        self._build(Conv1d(k, 64, Linear), k, Linear, pool, affine)
        self.k = k

    def forward(self, x):
        return self.head(self.point_part(x), self.k)


class BiPointNetEncoder(nn.Module):
    def __init__(self, Linear, global_feat=True, feature_transform=False, channel=3, pool="max", affine=True, tnet=True, bi_first=False,
                 use_bn=True):
        super().__init__()
        self.tnet = tnet
        if self.tnet:
            self.stn = BiSTN3d(channel, Linear, pool=pool, affine=affine, bi_first=bi_first)
        self.conv1 = Conv1d(channel, 64, Linear if bi_first else nn.Linear)
        self.conv2 = Conv1d(64, 128, Linear)
        self.conv3 = Conv1d(128, 1024, Linear)
        self.bn1 = nn.BatchNorm1d(64, affine=affine)
        self.bn2 = nn.BatchNorm1d(128, affine=affine)
        self.bn3 = nn.BatchNorm1d(1024, affine=affine)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if self.tnet and self.feature_transform:
            self.fstn = BiSTNkd(k=64, Linear=Linear, pool=pool, affine=affine, bi_first=bi_first)
        self.pool = pool
        self.use_bn = use_bn

    def forward(self, x):
        B, D, N = x.size()
        trans = self.stn(x) if self.tnet else None
        x = x.transpose(2, 1)
        feature = None
        if D == 6:
            x, feature = x.split(3, dim=2)
        elif D == 9:
            x, feature = x.split([3, 6], dim=2)
        if self.tnet:
            x = torch.bmm(x, trans)
        if D > 3:
            x = torch.cat([x, feature], dim=2)
        x = x.transpose(2, 1)
        x = F.hardtanh(self.bn1(self.conv1(x)) if self.use_bn else self.conv1(x))

        if self.tnet and self.feature_transform:
            trans_feat = self.fstn(x)
            x = torch.bmm(x.transpose(2, 1), trans_feat).transpose(2, 1)
        else:
            trans_feat = None

        pointfeat = x
        if self.use_bn:
            x = F.hardtanh(self.bn2(self.conv2(x)))
            x = self.bn3(self.conv3(x))
        else:
            x = F.hardtanh(self.conv2(x))
            x = self.conv3(x)

        if self.pool == "max":
            x = torch.max(x, 2, keepdim=True)[0]
        elif self.pool == "mean":
            x = torch.mean(x, 2, keepdim=True)
        elif self.pool == "ema-max":
            x = torch.max(x, 2, keepdim=True)[0] + (offset_map[N] if self.use_bn else -0.3)
        x = x.view(-1, 1024)
        if self.global_feat:
            return x, trans, trans_feat
        x = x.view(-1, 1024, 1).repeat(1, 1, N)
        return torch.cat([x, pointfeat], 1), trans, trans_feat


class BasicBiPointNet(nn.Module):
    def __init__(self, k=40, Linear=BiLinearLSR, pool="max", affine=True, tnet=True, bi_first=False, bi_last=False, use_bn=True):
        super().__init__()
        self.feat = BiPointNetEncoder(Linear, global_feat=True, feature_transform=True, channel=3, pool=pool, affine=affine, tnet=tnet,
                                      bi_first=bi_first, use_bn=use_bn)
        self.fc1 = Linear(1024, 512)
        self.fc2 = Linear(512, 256)
        self.fc3 = Linear(256, k) if bi_last else nn.Linear(256, k)
        self.use_bn = use_bn
        self.bn1 = nn.BatchNorm1d(512, affine=affine)
        self.bn2 = nn.BatchNorm1d(256, affine=affine)

    def head(self, x):
        """The encoder's [B,1024] -> the logits."""
        if self.use_bn:
            x = F.hardtanh(self.bn1(self.fc1(x)))
            x = F.hardtanh(self.bn2(self.fc2(x)))
        else:
            x = F.hardtanh(self.fc1(x))
            x = F.hardtanh(self.fc2(x))
        return self.fc3(x)

    def forward(self, x):
        x, trans, trans_feat = self.feat(x)
        return self.head(x), trans_feat


class BiPointNetLSREMax(BasicBiPointNet):
    """models.BiPointNet_CLS: BiLinearLSR layers, 'ema-max' pooling.  `args` is accepted and not read, as in the reference; the
    reference also ignores num_class (its head is always 40 wide) - here it sets the head's width, which is the same model at 40."""

    def __init__(self, args, num_class=40):
        super().__init__(k=num_class, Linear=BiLinearLSR, pool="ema-max")
