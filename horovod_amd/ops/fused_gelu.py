"""Fused bias + GELU + dropout backed by the CDNA4 kernels in
csrc/gelu_kernels.hip: out = dropout(gelu(x + bias), p), the middle of a
transformer feed-forward when x comes out of a bias-free GEMM.

Forward is one kernel that reads x once and writes out once; backward is one
pass over dy and x that recomputes x + bias and the mask, writes dx and keeps
the column sums for the bias gradient, plus a small fold when the launch had
more than one row chunk.  Nothing but x and the bias is saved.  The dropout
mask is the one of the fused LayerNorm kernels (docs/api.md, "Fused
LayerNorm"): a function of (seed, offset, element index), with seed and offset
from the device's default torch generator, which every call with p > 0
advances by 4.

Input the kernels do not take (CPU tensors, a last dimension that is not a
multiple of 8, non-contiguous or misaligned tensors, other dtypes, p > 0 while
a stream is capturing) goes through the composite
F.dropout(F.gelu(x + bias, approximate=...), p, training).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from horovod_amd import _core
from horovod_amd.ops.fused_ln import (_DTYPES, _act_ok, _check_p, _next_philox,
                                      _param_ok)

_APPROXIMATE = ("none", "tanh")


def _composite(x, bias, p, training, approximate):
    if bias is not None:
        x = x + bias
    return F.dropout(F.gelu(x, approximate=approximate), p, training)


def _eligible(x, bias, drop):
    """True when the native kernels take this call."""
    if not (x.is_cuda and x.dtype in _DTYPES and x.dim() >= 1):
        return False
    N = x.shape[-1]
    if N % 8 != 0 or N < 8 or x.numel() == 0 or not _act_ok(x):
        return False
    if not _param_ok(bias, x) or (bias is not None and bias.shape != (N,)):
        return False
    # the generator's state cannot be read on the host while capturing
    if drop and torch.cuda.is_current_stream_capturing():
        return False
    return True


class _FusedBiasGeluFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, bias, p, tanh):
        seed, offset = _next_philox(x.device) if p > 0.0 else (0, 0)
        ctx.p, ctx.seed, ctx.offset, ctx.tanh = p, seed, offset, tanh
        ctx.save_for_backward(x, bias)
        return _core.fused_bias_gelu_forward(x, bias, p, seed, offset, tanh)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        need_x, need_b = ctx.needs_input_grad[:2]
        # the forward checked its inputs; the incoming gradient can still be
        # strided, or a contiguous view at an offset the 16-B loads cannot take
        dy = dy.contiguous()
        if dy.data_ptr() % 16 != 0:
            dy = dy.clone()
        dx, dbias = _core.fused_bias_gelu_backward(
            dy, x, bias, ctx.p, ctx.seed, ctx.offset, ctx.tanh, need_b)
        if need_b:
            dbias = dbias.to(bias.dtype)
        return dx if need_x else None, dbias, None, None


def _check_approximate(approximate):
    if approximate not in _APPROXIMATE:
        raise ValueError(
            f"approximate has to be 'none' or 'tanh', but got {approximate!r}")
    return approximate


def bias_gelu_dropout(x, bias=None, p=0.0, training=True, approximate="none"):
    """dropout(gelu(x + bias, approximate), p) with bias over x's last
    dimension.  With training False, or p == 0, nothing is dropped."""
    p = _check_p(p)
    _check_approximate(approximate)
    drop = p if training else 0.0
    if _eligible(x, bias, drop > 0.0):
        return _FusedBiasGeluFn.apply(x, bias, drop, approximate == "tanh")
    return _composite(x, bias, p, training, approximate)


class FusedLinearGELU(nn.Linear):
    """dropout(gelu(linear(x)), p): the GEMM runs without its bias, and bias,
    GELU and dropout are one kernel pass.  Parameters and state_dict keys are
    nn.Linear's."""

    def __init__(self, in_features, out_features, bias=True, device=None,
                 dtype=None, p=0.0, approximate="none"):
        super().__init__(in_features, out_features, bias=bias, device=device,
                         dtype=dtype)
        self.p = _check_p(p)
        self.approximate = _check_approximate(approximate)

    def forward(self, input):
        return bias_gelu_dropout(F.linear(input, self.weight), self.bias,
                                 self.p, self.training, self.approximate)

    def extra_repr(self):
        return (super().extra_repr() +
                f", p={self.p}, approximate={self.approximate!r}")
