"""Scaffold shared by FusedSGD, FusedAdamW and FusedLAMB.

FusedOptimizer owns the max_grad_norm option, `last_grad_norm`, the group
defaults a foreign state dict may lack, and the step() skeleton: closure, one
GradClip over all groups, then per group the split into parameters the
kernels take (CUDA fp32 with a dense gradient) and parameters that take the
eager update, with a one-time warning so a benchmarked configuration cannot
silently lose the fusion.  A subclass supplies `_eager_update(p, group, clip)`
and `_fused_update(params, group, coef)`, its `_core.fused_*` call.
Every option stays in `param_groups`: hvd.DistributedOptimizer rebuilds the
optimizer from those alone.
"""
import warnings

import torch

from horovod_amd.ops import clip as _clip


class FusedOptimizer(torch.optim.Optimizer):
    # group keys a loaded state dict (e.g. torch.optim.AdamW's) may lack
    _GROUP_DEFAULTS = {"max_grad_norm": None}

    def __init__(self, params, defaults):
        _clip.check_max_grad_norm(defaults["max_grad_norm"])
        super().__init__(params, defaults)
        for group in self.param_groups:   # values given per param group
            _clip.check_max_grad_norm(group["max_grad_norm"])
        self.last_grad_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for key, value in self._GROUP_DEFAULTS.items():
                group.setdefault(key, value)

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
            fused = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._begin_param(p)
                g = p.grad
                # the kernels walk memory order: same layout, or not fused
                if p.is_cuda and p.dtype == torch.float32 and \
                        not g.is_sparse and (g.stride() == p.stride() or (
                            g.is_contiguous() and p.is_contiguous())):
                    fused.append(p)
                    continue
                if not getattr(self, "_warned_eager_fallback", False):
                    self._warned_eager_fallback = True
                    warnings.warn(
                        f"{type(self).__name__}: parameter is not CUDA fp32 "
                        "with a dense gradient of its own layout; using the "
                        "eager (unfused) update for such parameters")
                self._eager_update(p, group, clip)
            if fused:
                self._fused_update(
                    fused, group,
                    clip.kernel_coef(fused[0].device) if clip else None)
        return loss

    def _begin_param(self, p):
        """Bookkeeping of a parameter with a gradient, before its update."""

    @staticmethod
    def _eager_grad(p, clip):
        """p.grad as the eager updates consume it: dense and clipped."""
        g = p.grad.to_dense() if p.grad.is_sparse else p.grad
        return g if clip is None else clip.scaled(g)


class FusedMomentOptimizer(FusedOptimizer):
    """torch.optim.AdamW's state keys, for FusedAdamW and FusedLAMB."""

    def __init__(self, params, defaults):
        betas = defaults["betas"]
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas: {betas}")
        super().__init__(params, defaults)

    def _begin_param(self, p):
        st = self.state[p]
        if "step" not in st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        st["step"] += 1

    def _moments(self, p):
        """-> step as an int (AdamW state dicts hold a tensor), m, v"""
        st = self.state[p]
        return int(st["step"]), st["exp_avg"], st["exp_avg_sq"]

    def _by_step(self, params):
        """(step, params, grads, exp_avgs, exp_avg_sqs) per step count: a
        launch applies ONE bias correction; restored parameters can differ."""
        by_step = {}
        for p in params:
            step, m, v = self._moments(p)
            by_step.setdefault(step, []).append((p, p.grad, m, v))
        return [(step, *map(list, zip(*ts))) for step, ts in by_step.items()]
