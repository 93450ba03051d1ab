"""Fused softmax cross-entropy backed by the CDNA4 kernels in
csrc/xent_kernels.hip: F.cross_entropy over [M, V] logits that reads the
logits once in the forward, and reads them once and writes their gradient
once in the backward.  No softmax, no log-softmax and no fp32 copy of the
logits is ever stored; what the forward keeps for the backward is one fp32
log-sum-exp per row.

The logits go in as they are: under bf16 autocast F.cross_entropy first casts
them to fp32, here the kernels read the bf16 values and do their arithmetic in
fp32.  The loss is fp32 whatever the logits' dtype (F.cross_entropy returns
the logits' dtype outside autocast); the gradient has the logits' dtype and is
rounded once.

Native when the logits are a contiguous, 16-byte aligned 2-D fp32 / fp16 /
bf16 GPU tensor with at least one element and the labels a contiguous int64
[M] tensor on the same device.  Everything else (CPU tensors, other ranks,
class-probability targets, other label dtypes) is
F.cross_entropy(logits.float(), labels, ...).  There are no class weights.

bias: a [V] tensor added to every row of the logits inside the kernels
(csrc/xent_bias_kernels.hip), in fp32, so that the loss is that of logits +
bias without the sum ever being stored: under autocast a bf16 GEMM output
plus an fp32 bias parameter is an fp32 [M, V] tensor, and so is its gradient.
The backward returns the bias gradient next to the logits' (fp32 column sums
of the unrounded gradient, cast only for a bias that is not fp32).  Native
when the logits and labels are as above and the bias is a contiguous [V]
floating-point tensor on the same device; everything else is
F.cross_entropy(logits.float() + bias.float(), labels, ...).

Labels: ignore_index rows have loss 0 and a zero gradient row, and do not
count in the mean; with every row ignored 'mean' is NaN, as in torch.  A label
that is neither ignore_index nor in [0, V) makes that row's loss and gradient
NaN (torch raises a device-side assert there).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from horovod_amd import _core
from horovod_amd.ops.fused_ln import _DTYPES

_REDUCTIONS = ("none", "mean", "sum")


def _eligible(logits, labels):
    """True when the native kernels take this call."""
    return (torch.is_tensor(logits) and torch.is_tensor(labels) and
            logits.is_cuda and logits.dtype in _DTYPES and
            logits.dim() == 2 and logits.numel() > 0 and
            logits.is_contiguous() and logits.data_ptr() % 16 == 0 and
            labels.dtype == torch.int64 and labels.device == logits.device and
            labels.shape == logits.shape[:1] and labels.is_contiguous())


class _FusedXentFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, logits, labels, smoothing, ignore_index, reduction):
        loss, _, lse, count = _core.fused_xent_forward(
            logits, labels, smoothing, ignore_index, reduction)
        ctx.args = (smoothing, ignore_index, reduction)
        ctx.save_for_backward(logits, labels, lse, count)
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dloss):
        logits, labels, lse, count = ctx.saved_tensors
        # as in fused_gelu.py: the incoming gradient can be strided, or a
        # contiguous view at an odd offset
        dloss = dloss.float().contiguous()
        if dloss.data_ptr() % 16 != 0:
            dloss = dloss.clone()
        dx = _core.fused_xent_backward(dloss, logits, labels, lse, count,
                                       *ctx.args)
        return dx, None, None, None, None


def _bias_eligible(logits, bias):
    return (torch.is_tensor(bias) and bias.device == logits.device and
            bias.is_floating_point() and bias.shape == logits.shape[1:] and
            bias.is_contiguous())


class _FusedXentBiasFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, logits, bias, labels, smoothing, ignore_index,
                reduction):
        ctx.bias_dtype = bias.dtype
        bias = bias.detach().float()
        loss, _, lse, count = _core.fused_xent_bias_forward(
            logits, bias, labels, smoothing, ignore_index, reduction)
        ctx.args = (smoothing, ignore_index, reduction)
        ctx.save_for_backward(logits, bias, labels, lse, count)
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dloss):
        logits, bias, labels, lse, count = ctx.saved_tensors
        dloss = dloss.float().contiguous()
        if dloss.data_ptr() % 16 != 0:
            dloss = dloss.clone()
        dx, dbias = _core.fused_xent_bias_backward(
            dloss, logits, bias, labels, lse, count, *ctx.args)
        return dx, dbias.to(ctx.bias_dtype), None, None, None, None


def _check(label_smoothing, reduction):
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError("label_smoothing has to be in [0, 1), but got "
                         f"{label_smoothing}")
    if reduction not in _REDUCTIONS:
        raise ValueError("reduction has to be 'none', 'mean' or 'sum', but "
                         f"got {reduction!r}")
    return float(label_smoothing), reduction


def softmax_cross_entropy(logits, labels, label_smoothing=0.0,
                          ignore_index=-100, reduction="mean", bias=None):
    """F.cross_entropy(logits, labels, ...) without class weights, as an fp32
    loss for every logits dtype; with a bias [V], the loss of logits +
    bias."""
    label_smoothing, reduction = _check(label_smoothing, reduction)
    if bias is not None:
        if _eligible(logits, labels) and _bias_eligible(logits, bias):
            return _FusedXentBiasFn.apply(logits, bias, labels,
                                          label_smoothing, int(ignore_index),
                                          reduction)
        # F.cross_entropy keeps the classes in dimension 1
        bias = bias.float().view(-1, *[1] * max(logits.dim() - 2, 0))
        return F.cross_entropy(logits.float() + bias, labels,
                               ignore_index=ignore_index, reduction=reduction,
                               label_smoothing=label_smoothing)
    if _eligible(logits, labels):
        return _FusedXentFn.apply(logits, labels, label_smoothing,
                                  int(ignore_index), reduction)
    return F.cross_entropy(logits.float(), labels, ignore_index=ignore_index,
                           reduction=reduction,
                           label_smoothing=label_smoothing)


class FusedCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss under its argument names, without `weight`."""

    def __init__(self, label_smoothing=0.0, ignore_index=-100,
                 reduction="mean"):
        super().__init__()
        self.label_smoothing, self.reduction = _check(label_smoothing,
                                                      reduction)
        self.ignore_index = ignore_index

    def forward(self, input, target, bias=None):
        return softmax_cross_entropy(input, target, self.label_smoothing,
                                     self.ignore_index, self.reduction, bias)

    def extra_repr(self):
        return (f"label_smoothing={self.label_smoothing}, "
                f"ignore_index={self.ignore_index}, "
                f"reduction={self.reduction!r}")
