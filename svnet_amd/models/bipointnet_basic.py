"""The binary layer of the BiPointNet baseline (the reference's models/bipointnet_basic.py, itself from github.com/htqin/BiPointNet):
`BinaryQuantize` and `BiLinearLSR`, plain torch, train and eval, any device.  Names, constructor signatures and state_dict keys are the
reference's, so its checkpoints load with strict=True, and the operations run in its order, so the CPU results are its bits.

    BinaryQuantize   sign() forward (sign(0) = 0: ternary), a straight-through estimator backward that is zero where |input| > 1.
    BiLinearLSR      a Linear (no bias by default) whose weight is centred by its global mean, binarized and multiplied by one learnt
                     scalar `scale`; with binary_act the input is binarized too.  `scale` starts as 0, which means "not yet set": the
                     first forward sets it from its own input (reset_scale), the ratio of the standard deviations of the real and the
                     binarized product - or of the weights alone when the input is all zero and that ratio is NaN.

Not ported, because BiPointNet_CLS uses none of them: MeanShift, the XNOR / IRNet / BiReal variants of the layer and the plain BiLinear,
the BiConv1d* classes and the MLP helpers (MLP, BiMLP, BwMLP, FirstBiMLP).

forward() reads `scale.item()` on every call - the reference's first-call test - so the module can never be captured into a graph;
svnet_amd.bi_fused.FusedBiPointNet is the eval forward that can.
"""
import torch
import torch.nn.functional as F
from torch.nn import Parameter

__all__ = ["BinaryQuantize", "BiLinearLSR"]


class BinaryQuantize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input):
        ctx.save_for_backward(input)
        return torch.sign(input)

    @staticmethod
    def backward(ctx, grad_output):
        x, = ctx.saved_tensors
        grad_input = grad_output                     # (in place, as the reference does it)
        grad_input[x.gt(1)] = 0
        grad_input[x.lt(-1)] = 0
        return grad_input


class BiLinearLSR(torch.nn.Linear):
    def __init__(self, in_features, out_features, bias=False, binary_act=True):
        super().__init__(in_features, out_features, bias=bias)
        self.binary_act = binary_act
        # a 0-dim parameter, so that the key is in the state_dict before the first forward has set it
        self.register_parameter("scale", Parameter(torch.Tensor([0.0]).squeeze()))

    def reset_scale(self, input):
        bw = self.weight
        bw = bw - bw.mean()
        real, binary = F.linear(input, bw), F.linear(torch.sign(input), torch.sign(bw))
        self.scale = Parameter((real.std() / binary.std()).float().to(input.device))
        if torch.isnan(self.scale):                  # an all-zero input: 0 / 0
            self.scale = Parameter((bw.std() / torch.sign(bw).std()).float().to(input.device))

    def forward(self, input):
        bw = self.weight
        ba = input
        bw = bw - bw.mean()
        if self.scale.item() == 0.0:
            self.reset_scale(input)
        bw = BinaryQuantize.apply(bw)
        bw = bw * self.scale
        if self.binary_act:
            ba = BinaryQuantize.apply(ba)
        return F.linear(ba, bw)
