"""FusedAdamW: AdamW with moments + decoupled decay + update fused into one
CDNA4 kernel launch per 48-tensor bucket (csrc/adamw_kernels.hip).

Torch-eager AdamW issues ~8 kernels per parameter; a BERT-large step spends
several ms in them.  Drop-in for torch.optim.AdamW (state_dict-compatible, a
tensor-valued `step` included); CPU, non-fp32 or sparse-gradient parameters
take a correct eager fallback with a one-time warning, like FusedSGD.

max_grad_norm=<float> clips by the global L2 norm of all gradients inside
step(), replacing the synchronize / clip_grad_norm_ / skip_synchronize
recipe: one native multi-tensor norm pass (csrc/clip_kernels.hip), then the
step kernel multiplies each gradient by the coefficient as it reads it.
p.grad is left unscaled; the pre-clip norm is kept in `last_grad_norm`.

master_weights=True keeps an fp32 `master_param` and fp32 moments for every
fp16/bf16 parameter; the kernel updates the master and writes it, rounded to
nearest-even, into the parameter in the same pass (see _fused_base.py).

loss_scale="dynamic" (or a number for a static scale) makes the optimizer
its own loss scaler for fp16 training: backward runs on
`opt.scale_loss(loss)`; step() finds an overflow in one norm pass, unscales
inside the step kernel and skips the whole step on the device, without a
host read before the update (see _fused_base.py and loss_scale.py).
torch.amp.GradScaler.step(opt) is served by the same kernels.
"""
from horovod_amd import _core
from horovod_amd.ops._fused_base import FusedMomentOptimizer


class FusedAdamW(FusedMomentOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, max_grad_norm=None, master_weights=False,
                 loss_scale=None, loss_scale_args=None):
        super().__init__(params, dict(
            lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
            max_grad_norm=max_grad_norm, master_weights=master_weights,
            loss_scale=loss_scale, loss_scale_args=loss_scale_args))

    def _fused_update(self, params, group, coef, master, skip):
        b1, b2 = group["betas"]
        for step, ws, grads, avgs, sqs, models in self._by_step(params,
                                                                 master):
            _core.fused_adamw_step(ws, grads, avgs, sqs, group["lr"], b1, b2,
                                   group["eps"], group["weight_decay"], step,
                                   coef, models, skip)

    def _eager_update(self, p, w, g, group):
        """w: the tensor to update (p, or its fp32 master); g: the dense,
        clipped gradient in w's dtype."""
        b1, b2 = group["betas"]
        step, m, v = self._moments(p)
        w.mul_(1 - group["lr"] * group["weight_decay"])
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - b1 ** step
        bc2 = 1 - b2 ** step
        denom = (v.sqrt() / (bc2 ** 0.5)).add_(group["eps"])
        w.addcdiv_(m, denom, value=-group["lr"] / bc1)
