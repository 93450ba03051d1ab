"""FusedLAMB: LAMB (layer-wise adaptive moments, You et al. 2019) on three
CDNA4 kernel launches per 48-tensor bucket (csrc/lamb_kernels.hip).

For each parameter p with gradient g, moments m, v and step count t:

    g'    = g * coef                   # global clip coefficient, 1 if unset
    m     = b1*m + (1-b1)*g'
    v     = b2*v + (1-b2)*g'*g'
    mhat  = m / (1 - b1^t)   vhat = v / (1 - b2^t)   # 1 w/o bias_correction
    u     = mhat / (sqrt(vhat) + eps) + weight_decay * p
    trust = |p| / |u|  if (weight_decay != 0 or always_adapt)
                          and |p| > 0 and |u| > 0    # false for NaN
            1          otherwise
    p     = p - lr * trust * u

An eager LAMB is ~15 kernels and two norm launches per parameter.  Here one
launch updates the moments and reduces p*p and u*u per 8192-element chunk,
one turns each tensor's partials into its trust ratio, one applies the
update.  The sums run in a fixed order without atomics, so data-parallel
ranks, which hold replicated parameters and averaged gradients, derive
bitwise the same ratios without a collective.

State keys are those of torch.optim.AdamW / FusedAdamW, whose state dicts
load.  CPU, non-fp32 or sparse-gradient parameters take an eager update of
the same definition with a one-time warning.

max_grad_norm=<float> clips by the global L2 norm of all gradients inside
step(), as in FusedAdamW: one native norm pass over all groups, the
coefficient applied by the step kernel as it reads the gradient.  p.grad is
left unscaled; the pre-clip norm is kept in `last_grad_norm`.

master_weights=True keeps an fp32 `master_param` and fp32 moments for every
fp16/bf16 parameter.  p in the definition above is then the master: norms and
trust ratios are the master's, and the last launch writes the master and,
rounded to nearest-even, the parameter (see _fused_base.py).

loss_scale="dynamic" (or a number for a static scale) makes the optimizer
its own loss scaler for fp16 training: backward runs on
`opt.scale_loss(loss)`; step() finds an overflow in one norm pass, unscales
inside the moments kernel (g' above is then g * clip / scale) and skips the whole step on the device, without a
host read before the update (see _fused_base.py and loss_scale.py).
torch.amp.GradScaler.step(opt) is served by the same kernels.
"""
import torch

from horovod_amd import _core
from horovod_amd.ops._fused_base import FusedMomentOptimizer


class FusedLAMB(FusedMomentOptimizer):
    _GROUP_DEFAULTS = dict(FusedMomentOptimizer._GROUP_DEFAULTS,
                           bias_correction=True, always_adapt=False)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                 weight_decay=0.01, bias_correction=True, always_adapt=False,
                 max_grad_norm=None, master_weights=False, loss_scale=None,
                 loss_scale_args=None):
        super().__init__(params, dict(
            lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
            bias_correction=bias_correction, always_adapt=always_adapt,
            max_grad_norm=max_grad_norm, master_weights=master_weights,
            loss_scale=loss_scale, loss_scale_args=loss_scale_args))

    def _fused_update(self, params, group, coef, master, skip):
        b1, b2 = group["betas"]
        adapt = group["weight_decay"] != 0 or group["always_adapt"]
        for step, ws, grads, avgs, sqs, models in self._by_step(params,
                                                                 master):
            _core.fused_lamb_step(ws, grads, avgs, sqs, group["lr"], b1, b2,
                                  group["eps"], group["weight_decay"], step,
                                  group["bias_correction"], adapt, coef,
                                  models, skip)

    def _eager_update(self, p, w, g, group):
        """w: the tensor to update (p, or its fp32 master); g: the dense,
        clipped gradient in w's dtype."""
        b1, b2 = group["betas"]
        step, m, v = self._moments(p)
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = bc2 = 1.0
        if group["bias_correction"]:
            bc1 = 1 - b1 ** step
            bc2 = 1 - b2 ** step
        # 16-bit parameters: u and the two norms in fp32
        acc = w.dtype if w.dtype in (torch.float32, torch.float64) \
            else torch.float32
        wa = w.to(acc)
        u = (m.to(acc) / bc1) / ((v.to(acc) / bc2).sqrt_().add_(group["eps"]))
        u.add_(wa, alpha=group["weight_decay"])
        if group["weight_decay"] != 0 or group["always_adapt"]:
            w_norm = torch.linalg.vector_norm(wa)
            u_norm = torch.linalg.vector_norm(u)
            # 0-dim tensors, no host read; the compares are false for NaN
            trust = torch.where((w_norm > 0) & (u_norm > 0),
                                w_norm / u_norm, torch.ones_like(w_norm))
            u.mul_(trust)
        w.sub_(u.to(w.dtype), alpha=group["lr"])
