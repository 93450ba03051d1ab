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
"""
import warnings

import torch

from horovod_amd import _core
from horovod_amd.ops import clip as _clip


class FusedLAMB(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                 weight_decay=0.01, bias_correction=True, always_adapt=False,
                 max_grad_norm=None):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas: {betas}")
        _clip.check_max_grad_norm(max_grad_norm)
        # in defaults, hence in every param group: hvd.DistributedOptimizer
        # rebuilds the optimizer from param_groups alone
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay,
                        bias_correction=bias_correction,
                        always_adapt=always_adapt,
                        max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        for group in self.param_groups:   # values given per param group
            _clip.check_max_grad_norm(group["max_grad_norm"])
        self.last_grad_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("bias_correction", True)
            group.setdefault("always_adapt", False)
            group.setdefault("max_grad_norm", None)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = None
        max_grad_norm = _clip.group_max_grad_norm(self.param_groups)
        if max_grad_norm is not None:
            clip = _clip.GradClip(
                [p.grad for group in self.param_groups
                 for p in group["params"] if p.grad is not None],
                max_grad_norm)
            self.last_grad_norm = clip.total_norm
        for group in self.param_groups:
            # bucket by bias-correction step: the fused launch applies ONE
            # step factor, and params restored mid-run can disagree
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state.setdefault(p, {})
                if "step" not in st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                if not p.is_cuda or p.dtype != torch.float32 or \
                        p.grad.is_sparse:
                    if not getattr(self, "_warned_eager_fallback", False):
                        self._warned_eager_fallback = True
                        warnings.warn(
                            "FusedLAMB: parameter is not CUDA fp32; using "
                            "the eager (unfused) update for such parameters")
                    self._eager_update(p, group, st, clip)
                    continue
                # torch.optim.AdamW state dicts carry the step as a tensor
                b = by_step.setdefault(int(st["step"]), ([], [], [], []))
                b[0].append(p)
                b[1].append(p.grad)
                b[2].append(st["exp_avg"])
                b[3].append(st["exp_avg_sq"])
            b1, b2 = group["betas"]
            adapt = group["weight_decay"] != 0 or group["always_adapt"]
            for step_t, (params, grads, avgs, sqs) in by_step.items():
                _core.fused_lamb_step(params, grads, avgs, sqs,
                                      group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"], step_t,
                                      group["bias_correction"], adapt,
                                      clip.kernel_coef(params[0].device)
                                      if clip else None)
        return loss

    def _eager_update(self, p, group, st, clip=None):
        b1, b2 = group["betas"]
        g = p.grad
        if g.is_sparse:
            g = g.to_dense()
        if clip is not None:
            g = clip.scaled(g)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = bc2 = 1.0
        if group["bias_correction"]:
            bc1 = 1 - b1 ** int(st["step"])
            bc2 = 1 - b2 ** int(st["step"])
        # 16-bit parameters: u and the two norms in fp32
        acc = p.dtype if p.dtype in (torch.float32, torch.float64) \
            else torch.float32
        w = p.to(acc)
        u = (m.to(acc) / bc1) / ((v.to(acc) / bc2).sqrt_().add_(group["eps"]))
        u.add_(w, alpha=group["weight_decay"])
        if group["weight_decay"] != 0 or group["always_adapt"]:
            w_norm = torch.linalg.vector_norm(w)
            u_norm = torch.linalg.vector_norm(u)
            # 0-dim tensors, no host read; the compares are false for NaN
            trust = torch.where((w_norm > 0) & (u_norm > 0),
                                w_norm / u_norm, torch.ones_like(w_norm))
            u.mul_(trust)
        p.sub_(u.to(p.dtype), alpha=group["lr"])
