"""FusedLARS: LARS (layer-wise adaptive rate scaling, You et al. 2017; the
LARC of apex) on three CDNA4 kernel launches per 48-tensor bucket
(csrc/lars_kernels.hip).  It is momentum SGD whose step is scaled per tensor
by a trust ratio: the large-batch recipe for ResNet, as FusedLAMB is for BERT.

For each parameter p with gradient g and momentum buffer m (fp32, zeros when
created):

    g'    = g * coef                 # clip coefficient and/or 1/loss-scale;
                                     # 1 if unset
    wn    = |p|_2      gn = |g'|_2   # over the whole tensor
    adapt = weight_decay != 0 or always_adapt
    trust = trust_coefficient * wn / (gn + weight_decay * wn + eps)
                if adapt and wn > 0 and gn > 0       # false for NaN
            1   otherwise
    trust = min(trust / lr, 1)   if trust_clip and the adaptive branch was
                                 # taken (LARC "clip" mode; fp32, so lr == 0
                                 # gives 1)
    d     = trust * (g' + weight_decay * p)
    m     = momentum * m + d         # every step, the first included
    d'    = d + momentum * m   if nesterov   else m
    p     = p - lr * d'

There is no dampening, and the buffer is kept even with momentum == 0, so
there is one kernel path.  A group without weight decay (biases and BatchNorm
parameters, see split_decay_groups) has trust == 1: momentum SGD without
decay, the standard LARS exclusion.

An eager LARS is ~10 kernels and two norm launches per parameter.  Here one
launch reduces p*p and g'*g' per 8192-element chunk, one turns each tensor's
partials into its trust ratio, one applies the update.  The sums run in a
fixed order without atomics, so data-parallel ranks, which hold replicated
parameters and averaged gradients, derive bitwise the same ratios without a
collective.

The state key is `momentum_buffer`, so a torch.optim.SGD or FusedSGD state
dict loads.  CPU, non-fp32 or sparse-gradient parameters take an eager update
of the same definition with a one-time warning.

max_grad_norm, master_weights and loss_scale work as in the other fused
optimizers (see _fused_base.py).  With master_weights p above is the fp32
master: norms and trust ratios are the master's, and the last launch writes
the master and, rounded to nearest-even, the parameter.  The norm pass sums
in one order whatever the gradient's dtype, so master, buffer and ratios are
bitwise those of an fp32 FusedLARS fed the widened gradients.  With
max_grad_norm the clip's norm pass and the per-tensor norm pass both read the
gradients; sharing that read is not done.
"""
import torch

from horovod_amd import _core
from horovod_amd.ops._fused_base import FusedOptimizer, _fp32_like


class FusedLARS(FusedOptimizer):
    _GROUP_DEFAULTS = dict(FusedOptimizer._GROUP_DEFAULTS,
                           trust_coefficient=0.001, eps=1e-8,
                           trust_clip=False, always_adapt=False)

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0,
                 trust_coefficient=0.001, eps=1e-8, nesterov=False,
                 trust_clip=False, always_adapt=False, max_grad_norm=None,
                 master_weights=False, loss_scale=None,
                 loss_scale_args=None):
        defaults = dict(
            lr=lr, momentum=momentum, weight_decay=weight_decay,
            trust_coefficient=trust_coefficient, eps=eps, nesterov=nesterov,
            trust_clip=trust_clip, always_adapt=always_adapt,
            max_grad_norm=max_grad_norm, master_weights=master_weights,
            loss_scale=loss_scale, loss_scale_args=loss_scale_args)
        self._check_group(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:   # values given per param group
            self._check_group(group)

    @staticmethod
    def _check_group(group):
        if not 0.0 <= group["momentum"] < 1.0:
            raise ValueError(f"invalid momentum: {group['momentum']}")
        if group["nesterov"] and group["momentum"] == 0:
            raise ValueError("nesterov requires momentum > 0")
        if group["trust_coefficient"] < 0:
            raise ValueError(
                f"invalid trust_coefficient: {group['trust_coefficient']}")
        if group["eps"] < 0:
            raise ValueError(f"invalid eps: {group['eps']}")

    def _begin_param(self, p, master):
        super()._begin_param(p, master)
        st = self.state[p]
        # torch.optim.SGD saves None before its first step
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = _fp32_like(p) if master \
                else torch.zeros_like(p)

    def _fused_update(self, params, group, coef, master, skip):
        ws = [self.state[p]["master_param"] for p in params] if master \
            else params
        adapt = group["weight_decay"] != 0 or group["always_adapt"]
        _core.fused_lars_step(
            ws, [p.grad for p in params],
            [self.state[p]["momentum_buffer"] for p in params], group["lr"],
            group["momentum"], group["weight_decay"],
            group["trust_coefficient"], group["eps"], group["nesterov"],
            group["trust_clip"], adapt, coef, params if master else None,
            skip)

    def _eager_update(self, p, w, g, group):
        """w: the tensor to update (p, or its fp32 master); g: the dense,
        clipped gradient in w's dtype."""
        wd, momentum = group["weight_decay"], group["momentum"]
        m = self.state[p]["momentum_buffer"]
        # 16-bit parameters: d and the two norms in fp32
        acc = w.dtype if w.dtype in (torch.float32, torch.float64) \
            else torch.float32
        wa, ga = w.to(acc), g.to(acc)
        d = ga.add(wa, alpha=wd)
        if wd != 0 or group["always_adapt"]:
            w_norm = torch.linalg.vector_norm(wa)
            g_norm = torch.linalg.vector_norm(ga)
            # 0-dim tensors, no host read; the compares are false for NaN
            trust = group["trust_coefficient"] * w_norm / (
                g_norm + wd * w_norm + group["eps"])
            if group["trust_clip"]:
                clipped = trust / group["lr"]
                trust = torch.where(clipped < 1, clipped,
                                    torch.ones_like(clipped))
            d.mul_(torch.where((w_norm > 0) & (g_norm > 0), trust,
                               torch.ones_like(trust)))
        m.mul_(momentum).add_(d.to(m.dtype))
        if group["nesterov"]:
            d.add_(m.to(acc), alpha=momentum)
        else:
            d = m
        w.sub_(d.to(w.dtype), alpha=group["lr"])
