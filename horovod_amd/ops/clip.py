"""Global-norm gradient clipping on the CDNA4 clip kernels
(csrc/clip_kernels.hip).

One multi-tensor pass computes {total_norm, coef} on the device without a
host synchronisation; the coefficient is then either applied in place by a
second multi-tensor kernel (`clip_grad_norm_`) or handed to the fused
optimizer step, which multiplies the gradient by it as it reads it
(`FusedSGD` / `FusedAdamW` / `FusedLAMB` with `max_grad_norm=`).

The norm reduces in a fixed order, so identical gradients give a bitwise
identical coefficient on every data-parallel rank.
"""
import torch

from horovod_amd import _core

_NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _dense(g):
    if g.is_contiguous():
        return True
    if g.dim() == 4:
        return g.is_contiguous(memory_format=torch.channels_last)
    if g.dim() == 5:
        return g.is_contiguous(memory_format=torch.channels_last_3d)
    return False


def native_eligible(grads):
    """True when the norm of `grads` can run on the native kernel: every
    gradient a dense CUDA fp32/bf16/fp16 tensor, all on one device."""
    if not grads:
        return False
    device = grads[0].device
    for g in grads:
        if not g.is_cuda or g.device != device or g.is_sparse or \
                g.dtype not in _NATIVE_DTYPES or not _dense(g):
            return False
    return True


def check_max_grad_norm(max_grad_norm):
    if max_grad_norm is not None and not max_grad_norm > 0:
        raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")


def group_max_grad_norm(param_groups):
    """The one max_grad_norm all param groups agree on (None = no clipping);
    the norm is global, so differing values have no meaning.  Values set
    through a param-group dict are validated here like the constructor's."""
    values = {g.get("max_grad_norm") for g in param_groups}
    for v in values:
        check_max_grad_norm(v)
    if len(values) > 1:
        raise ValueError(
            "max_grad_norm must be the same in every param group (the clip "
            f"is by the global norm), got {sorted(map(str, values))}")
    return values.pop() if values else None


def torch_norm(grads, fp32=False):
    """Global L2 norm of `grads` in torch ops, a 0-dim tensor on the device
    of the first: the path of CPU, sparse or multi-device gradients.  `fp32`:
    fp16/bf16 gradients are accumulated, and the norm returned, in fp32."""
    if not grads:
        return torch.zeros(())
    first = grads[0].device
    norms = []
    for g in grads:
        g = g.coalesce()._values() if g.is_sparse else g
        wide = torch.float32 if fp32 and g.dtype in (
            torch.float16, torch.bfloat16) else None
        norms.append(torch.linalg.vector_norm(g, 2.0, dtype=wide).to(first))
    return torch.linalg.vector_norm(torch.stack(norms), 2.0)


class GradClip:
    """Pre-clip norm and clip coefficient of one optimizer step.

    `total_norm` and the coefficients are 0-dim device tensors; nothing here
    reads them on the host.  The coefficient follows
    torch.nn.utils.clip_grad_norm_: min(max_norm / (total_norm + 1e-6), 1),
    NaN for a NaN norm and 0 for an infinite one.
    """

    def __init__(self, grads, max_norm):
        max_norm = float(max_norm)
        if native_eligible(grads):
            out = _core.multi_tensor_grad_norm(grads, max_norm)
            self.total_norm, coef = out[0], out[1]
        else:
            # CPU, sparse or multi-device gradients: same formula in torch ops
            coef = None
            self.total_norm = torch_norm(grads)
            if grads:
                coef = torch.clamp(max_norm / (self.total_norm + 1e-6),
                                   max=1.0)
        self._coef = {} if coef is None else {coef.device: coef}
        self._first = coef

    def coef(self, device):
        """The coefficient as a 0-dim tensor on `device` (None when there
        was no gradient at all)."""
        if self._first is None:
            return None
        c = self._coef.get(device)
        if c is None:
            c = self._coef[device] = self._first.to(device)
        return c

    def kernel_coef(self, device):
        """The coefficient in the form the fused step kernels take."""
        c = self.coef(device)
        return None if c is None else c.float()

    def scaled(self, g):
        """g * coef, out of place (0-dim coef: g keeps its dtype)."""
        c = self.coef(g.device)
        return g if c is None else g * c


def clip_grad_norm_(parameters, max_norm, norm_type=2.0,
                    error_if_nonfinite=False, foreach=None):
    """Drop-in for torch.nn.utils.clip_grad_norm_: scales the gradients of
    `parameters` in place so their global norm is at most `max_norm` and
    returns the pre-clip norm.

    One difference on the native path: the returned norm is always an fp32
    0-dim tensor.  torch returns it in the gradients' dtype, i.e. rounded to
    bf16/fp16 for half-precision gradients (and derives its coefficient from
    the rounded value); here norm and coefficient stay fp32.

    L2 norm over dense CUDA fp32/bf16/fp16 gradients on one device runs on
    two native multi-tensor kernels (norm, then in-place scale, which leaves
    memory untouched when nothing needs clipping) with no host
    synchronisation; everything else defers to torch's implementation.
    """
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if float(norm_type) == 2.0 and not error_if_nonfinite and \
            native_eligible(grads):
        out = _core.multi_tensor_grad_norm(grads, float(max_norm))
        _core.multi_tensor_scale_(grads, out[1])
        return out[0]
    return torch.nn.utils.clip_grad_norm_(
        parameters, max_norm, norm_type=norm_type,
        error_if_nonfinite=error_if_nonfinite, foreach=foreach)
