"""The reference's four custom modules (Normalize2.lua, Margin2.lua, StereoJoin1.lua, BCECriterion2.lua) over torch CUDA tensors.

`Normalize2` and `Margin2` sit on the operators of the adcensus table (Normalize_forward of libmcadcensus.so; Normalize_backward_input
and Margin2 of libmcops.so).  `StereoJoin1` and `BCECriterion2` are tensor arithmetic in the reference too, and are the same torch
operations in the same order here.  Each module has `forward` / `backward` as the reference's updateOutput / updateGradInput, and
keeps `output` / `gradInput` like an nn.Module of Torch7.  The `*_fn` wrappers are torch.autograd.Functions over them, so that the
modules compose with F.conv2d:

    loss = margin2_fn(stereo_join1_fn(normalize2_fn(F.conv2d(x, w, b))), 0.2, 1)

The fused trainers (train*.py) do not run through this file; tests hold their kernels' tails to it."""
import torch

from . import adcensus

EPS = 1e-12   # BCECriterion2.lua:3


class Normalize2:
    """nn.Normalize2: every pixel's feature vector divided by sqrt(sum of squares + 1e-5)."""

    def __init__(self):
        self.norm = self.output = self.gradInput = None

    def forward(self, input):
        N, _, H, W = input.shape
        self.norm = torch.empty((N, 1, H, W), dtype=torch.float32, device=input.device)
        self.output = torch.empty_like(input)
        adcensus.Normalize_forward(input, self.norm, self.output)
        return self.output

    def backward(self, input, gradOutput):
        self.gradInput = torch.empty_like(input)
        adcensus.Normalize_backward_input(gradOutput.contiguous(), input, self.norm, self.gradInput)
        return self.gradInput


class Margin2:
    """nn.Margin2(margin, pow): the hinge on (pos, neg) score pairs; output is the mean over the pairs as a 0-d device tensor
    (the reference's Lua number, without the read-back), gradInput is divided by the pair count."""

    def __init__(self, margin, pow):
        self.margin, self.pow = margin, pow
        self.tmp = self.output = self.gradInput = None

    def forward(self, input, target=None):
        assert input.dim() == 4 and tuple(input.shape[1:]) == (1, 1, 1) and input.shape[0] % 2 == 0
        self.tmp = torch.empty(input.shape[0] // 2, dtype=torch.float32, device=input.device)
        self.gradInput = torch.empty_like(input)
        adcensus.Margin2(input, self.tmp, self.gradInput, self.margin, self.pow)
        self.output = self.tmp.mean()
        self.gradInput.div_(self.tmp.shape[0])
        return self.output

    def backward(self, input, target=None):
        return self.gradInput


def _slice_input(input):
    """slice_input (StereoJoin1.lua:9-15): the even and the odd batch entries as views."""
    return input[0::2], input[1::2]


class StereoJoin1:
    """nn.StereoJoin1: the dot product of each (left, right) pair of feature maps over the channels, (2n,C,H,W) -> (n,1,H,W)."""

    def __init__(self):
        self.tmp = self.output = self.gradInput = None

    def forward(self, input):
        input_L, input_R = _slice_input(input)
        self.tmp = torch.mul(input_L, input_R)
        self.output = self.tmp.sum(1, keepdim=True)
        return self.output

    def backward(self, input, gradOutput):
        self.gradInput = torch.empty_like(input)
        input_L, input_R = _slice_input(input)
        gradInput_L, gradInput_R = _slice_input(self.gradInput)
        torch.mul(input_R, gradOutput.expand_as(input_R), out=gradInput_L)
        torch.mul(input_L, gradOutput.expand_as(input_L), out=gradInput_R)
        return self.gradInput


class BCECriterion2:
    """nn.BCECriterion2: -(log(input + eps) * target + log(1 - input + eps) * (1 - target)), averaged; eps is added after the
    subtraction, in fp32, in the reference's order."""

    def __init__(self):
        self.sizeAverage = True
        self.output = self.gradInput = None

    def forward(self, input, target):
        term1 = torch.ones_like(input).add_(target, alpha=-1)
        term2 = torch.ones_like(input).add_(input, alpha=-1).add_(EPS).log_().mul_(term1)
        term3 = input.clone().add_(EPS).log_().mul_(target)
        term3.add_(term2)
        if self.sizeAverage:
            term3.div_(target.numel())
        self.output = -term3.sum()
        return self.output

    def backward(self, input, target):
        term1 = torch.ones_like(input).add_(target, alpha=-1)
        term2 = torch.ones_like(input).add_(input, alpha=-1)
        term2.add_(EPS)
        term1.div_(term2)
        term3 = input.clone().add_(EPS)
        self.gradInput = target.clone().div_(term3)
        self.gradInput.add_(term1, alpha=-1)
        if self.sizeAverage:
            self.gradInput.div_(target.numel())
        self.gradInput.mul_(-1)
        return self.gradInput


class _Normalize2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input):
        m = Normalize2()
        input = input.contiguous()
        out = m.forward(input)
        ctx.module = m
        ctx.save_for_backward(input)
        return out

    @staticmethod
    def backward(ctx, grad):
        input, = ctx.saved_tensors
        return ctx.module.backward(input, grad)


class _StereoJoin1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input):
        ctx.save_for_backward(input)
        return StereoJoin1().forward(input)

    @staticmethod
    def backward(ctx, grad):
        input, = ctx.saved_tensors
        return StereoJoin1().backward(input, grad)


class _Margin2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, margin, pow):
        m = Margin2(margin, pow)
        out = m.forward(input.contiguous())
        ctx.save_for_backward(m.gradInput)
        return out

    @staticmethod
    def backward(ctx, grad):
        gradInput, = ctx.saved_tensors
        return gradInput * grad, None, None


class _BCECriterion2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target):
        ctx.save_for_backward(input, target)
        return BCECriterion2().forward(input, target)

    @staticmethod
    def backward(ctx, grad):
        input, target = ctx.saved_tensors
        return BCECriterion2().backward(input, target) * grad, None


normalize2_fn = _Normalize2Fn.apply
stereo_join1_fn = _StereoJoin1Fn.apply
margin2_fn = _Margin2Fn.apply
bce_criterion2_fn = _BCECriterion2Fn.apply
