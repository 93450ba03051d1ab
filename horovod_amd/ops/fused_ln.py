"""Fused dropout + residual add + LayerNorm backed by the CDNA4 kernels in
csrc/ln_kernels.hip: y = LayerNorm(residual + dropout(x)), the pattern that
closes both halves of a post-LN transformer layer.

Forward is one kernel with one read of x and of the residual; backward is one
pass over dy and z plus a small fold for the parameter gradients.  The dropout
mask is never stored: it is a function of (seed, offset, element index) that
forward and backward both evaluate (docs/api.md, "Fused LayerNorm").  Seed and
offset come from the device's default torch generator, which every call with
p > 0 advances by 4, so torch.manual_seed and torch.cuda.get_rng_state /
set_rng_state govern the mask.

Input the kernels do not take (CPU tensors, a row length that is not a
multiple of 8 or above 4096, a normalized_shape of more than one dimension,
non-contiguous or misaligned tensors, p > 0 while a stream is capturing) goes
through the composite F.layer_norm(residual + F.dropout(x)), so the modules
are drop-in and state_dict-compatible with nn.LayerNorm.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from horovod_amd import _core

MAX_H = 4096
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _composite(x, residual, normalized_shape, weight, bias, p, eps, training):
    if p > 0.0:
        x = F.dropout(x, p, training)
    if residual is not None:
        x = residual + x
    return F.layer_norm(x, normalized_shape, weight, bias, eps)


def _act_ok(t):
    return t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0


def _param_ok(w, x):
    return w is None or (w.is_cuda and w.device == x.device and
                         w.dtype in (torch.float32, x.dtype) and
                         w.is_contiguous() and w.data_ptr() % 16 == 0)


def _eligible(x, residual, normalized_shape, weight, bias, drop):
    """True when the native kernels take this call (residual already in x's
    dtype)."""
    if not (x.is_cuda and x.dtype in _DTYPES and len(normalized_shape) == 1):
        return False
    H = normalized_shape[0]
    if x.dim() < 1 or x.shape[-1] != H or H % 8 != 0 or not 8 <= H <= MAX_H:
        return False
    if x.numel() == 0 or not _act_ok(x):
        return False
    if residual is not None and not (
            residual.shape == x.shape and residual.dtype == x.dtype and
            residual.device == x.device and _act_ok(residual)):
        return False
    if not (_param_ok(weight, x) and _param_ok(bias, x)):
        return False
    # the generator's state cannot be read on the host while capturing
    if drop and torch.cuda.is_current_stream_capturing():
        return False
    return True


def _next_philox(device):
    """(seed, offset) of the device's default generator, which moves on by 4
    (one Philox call's worth) so the next call draws another mask."""
    index = device.index
    if index is None:
        index = torch.cuda.current_device()
    gen = torch.cuda.default_generators[index]
    seed = gen.initial_seed()
    offset = gen.get_offset()
    gen.set_offset(offset + 4)
    return seed, offset


class _FusedLNFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, residual, weight, bias, p, eps):
        seed, offset = _next_philox(x.device) if p > 0.0 else (0, 0)
        need_w = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        save_z = need_w or ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        y, z, mean, rstd = _core.fused_ln_forward(
            x, residual, weight, bias, p, eps, seed, offset, save_z)
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        ctx.has_residual = residual is not None
        ctx.bias_dtype = None if bias is None else bias.dtype
        if save_z:
            # z is x itself where the kernel had nothing to add to it
            ctx.save_for_backward(x if z is None else z, mean, rstd, weight)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy):
        z, mean, rstd, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        # the forward checked its inputs; the incoming gradient can still be
        # strided, or a contiguous view at an offset the 16-B loads cannot take
        dy = dy.contiguous()
        if dy.data_ptr() % 16 != 0:
            dy = dy.clone()
        dz, dx, dgamma, dbeta = _core.fused_ln_backward(
            dy, z, mean, rstd, weight, ctx.p, ctx.seed,
            ctx.offset, need[2] or need[3])
        if need[2]:
            dgamma = dgamma.to(weight.dtype)
        if need[3]:
            dbeta = dbeta.to(ctx.bias_dtype)
        return (dx if need[0] else None,
                dz if ctx.has_residual and need[1] else None,
                dgamma if need[2] else None, dbeta if need[3] else None,
                None, None)


def _check_p(p):
    if not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(
            f"dropout probability has to be between 0 and 1, but got {p}")
    return float(p)


def _normalized(x, weight, bias, normalized_shape):
    if normalized_shape is not None:
        return tuple(normalized_shape)
    for w in (weight, bias):
        if w is not None:
            return tuple(w.shape)
    return (x.shape[-1],)


def dropout_add_layer_norm(x, residual=None, weight=None, bias=None, p=0.0,
                           eps=1e-5, training=True, normalized_shape=None):
    """LayerNorm(residual + dropout(x, p)) over the trailing dimensions
    `normalized_shape` (default: the weight's shape, or x's last dimension).

    residual, weight and bias may be None.  A residual of another dtype is
    cast to x's.  With training False, or p == 0, nothing is dropped.
    """
    p = _check_p(p)
    shape = _normalized(x, weight, bias, normalized_shape)
    if residual is not None and residual.dtype != x.dtype:
        residual = residual.to(x.dtype)
    drop = p if training else 0.0
    if _eligible(x, residual, shape, weight, bias, drop > 0.0):
        return _FusedLNFn.apply(x, residual, weight, bias, drop, eps)
    return _composite(x, residual, shape, weight, bias, p, eps, training)


class FusedLayerNorm(nn.LayerNorm):
    """nn.LayerNorm whose GPU forward and backward are the fused kernels."""

    def forward(self, input):
        return dropout_add_layer_norm(
            input, None, self.weight, self.bias, 0.0, self.eps, self.training,
            self.normalized_shape)


class FusedDropoutAddLayerNorm(nn.LayerNorm):
    """LayerNorm(residual + dropout(x, p)) in one kernel pass; parameters and
    state_dict keys are nn.LayerNorm's.  Eval mode is the fused path with
    p = 0."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True,
                 bias=True, device=None, dtype=None, p=0.0):
        super().__init__(normalized_shape, eps=eps,
                         elementwise_affine=elementwise_affine, bias=bias,
                         device=device, dtype=dtype)
        self.p = _check_p(p)

    def forward(self, x, residual=None):
        return dropout_add_layer_norm(
            x, residual, self.weight, self.bias, self.p, self.eps,
            self.training, self.normalized_shape)

    def extra_repr(self):
        return super().extra_repr() + f", p={self.p}"
