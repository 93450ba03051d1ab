"""Scaffold shared by FusedSGD, FusedAdamW and FusedLAMB.

FusedOptimizer owns the max_grad_norm and master_weights options,
`last_grad_norm`, the group defaults a foreign state dict may lack, and the
step() skeleton: closure, one GradClip over all groups, then per group the
split into parameters the kernels take and parameters that take the eager
update, with a one-time warning so a benchmarked configuration cannot
silently lose the fusion.  The kernels take CUDA fp32 parameters with a dense
gradient of their own layout and, in a master_weights group, CUDA fp16/bf16
parameters with such a gradient of their own dtype.

master_weights=True gives every fp16/bf16 parameter of the group fp32 state:
`master_param`, made from p.float() when the parameter first has a gradient,
and fp32 moments.  The update runs on the master in fp32 and the parameter
is overwritten with the rounded master, so the master is authoritative: a
parameter changed from outside is not picked up.  fp32 parameters of the
group are updated as ever and get no master.

A subclass supplies `_eager_update(p, w, g, group)` and `_fused_update(params,
group, coef, master)`, its `_core.fused_*` call.  Every option stays in
`param_groups`: hvd.DistributedOptimizer rebuilds the optimizer from those
alone.
"""
import itertools
import warnings

import torch

from horovod_amd.ops import clip as _clip

_LOW_PRECISION = (torch.float16, torch.bfloat16)
# state that is fp32 for a master-weight parameter, whatever its own dtype
_MASTER_STATE_KEYS = ("master_param", "exp_avg", "exp_avg_sq",
                      "momentum_buffer")


def _fp32_like(p):
    """fp32 zeros in p's layout."""
    return torch.zeros_like(p, dtype=torch.float32)


class FusedOptimizer(torch.optim.Optimizer):
    # group keys a loaded state dict (e.g. torch.optim.AdamW's) may lack
    _GROUP_DEFAULTS = {"max_grad_norm": None, "master_weights": False}

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

    def load_state_dict(self, state_dict):
        """torch casts every floating state tensor to its parameter's dtype;
        the fp32 state of master-weight parameters is restored from the
        given dict instead, on the parameter's device."""
        super().load_state_dict(state_dict)
        saved_ids = itertools.chain.from_iterable(
            g["params"] for g in state_dict["param_groups"])
        for group in self.param_groups:
            for p, saved_id in zip(group["params"], saved_ids):
                if not self._has_master(p, group):
                    continue
                saved = state_dict["state"].get(saved_id, {})
                for key in _MASTER_STATE_KEYS:
                    if torch.is_tensor(saved.get(key)):
                        self.state[p][key] = saved[key].detach().to(
                            device=p.device, dtype=torch.float32, copy=True)

    @staticmethod
    def _has_master(p, group):
        return group["master_weights"] and p.dtype in _LOW_PRECISION

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
            fused, fused_master = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                master = self._has_master(p, group)
                self._begin_param(p, master)
                g = p.grad
                # the kernels walk memory order: same layout, or not fused
                if p.is_cuda and not g.is_sparse and (
                        g.dtype == p.dtype if master
                        else p.dtype == torch.float32) and (
                            g.stride() == p.stride() or (
                                g.is_contiguous() and p.is_contiguous())):
                    (fused_master if master else fused).append(p)
                    continue
                if not getattr(self, "_warned_eager_fallback", False):
                    self._warned_eager_fallback = True
                    warnings.warn(
                        f"{type(self).__name__}: parameter is not CUDA fp32 "
                        "(or, with master_weights, fp16/bf16) with a dense "
                        "gradient of its own layout; using the eager "
                        "(unfused) update for such parameters")
                g = g.to_dense() if g.is_sparse else g
                if master:
                    # fp32 arithmetic on the master, then the rounded copy
                    w = self.state[p]["master_param"]
                    g = g.float()
                    if clip is not None and clip.coef(g.device) is not None:
                        g = g * clip.coef(g.device).float()
                    self._eager_update(p, w, g, group)
                    p.copy_(w)
                else:
                    self._eager_update(
                        p, p, g if clip is None else clip.scaled(g), group)
            for params, master in ((fused, False), (fused_master, True)):
                if params:
                    self._fused_update(
                        params, group,
                        clip.kernel_coef(params[0].device) if clip else None,
                        master)
        return loss

    def _begin_param(self, p, master):
        """Bookkeeping of a parameter with a gradient, before its update;
        `master`: it is a master-weight parameter."""
        if not master:
            return
        st = self.state[p]
        if "master_param" not in st:
            st["master_param"] = p.detach().float()
        # state from a run without master weights
        for key in _MASTER_STATE_KEYS[1:]:
            if torch.is_tensor(st.get(key)) and \
                    st[key].dtype != torch.float32:
                st[key] = st[key].float()


class FusedMomentOptimizer(FusedOptimizer):
    """torch.optim.AdamW's state keys, for FusedAdamW and FusedLAMB."""

    def __init__(self, params, defaults):
        betas = defaults["betas"]
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas: {betas}")
        super().__init__(params, defaults)

    def _begin_param(self, p, master):
        super()._begin_param(p, master)
        st = self.state[p]
        if "step" not in st:
            st["step"] = 0
            st["exp_avg"] = _fp32_like(p) if master else torch.zeros_like(p)
            st["exp_avg_sq"] = _fp32_like(p) if master else torch.zeros_like(p)
        st["step"] += 1

    def _moments(self, p):
        """-> step as an int (AdamW state dicts hold a tensor), m, v"""
        st = self.state[p]
        return int(st["step"]), st["exp_avg"], st["exp_avg_sq"]

    def _by_step(self, params, master):
        """(step, params, grads, exp_avgs, exp_avg_sqs, model_params) per
        step count: a launch applies ONE bias correction; restored parameters
        can differ.  With `master`, params are the fp32 masters and
        model_params the parameters themselves; without, model_params is
        None."""
        by_step = {}
        for p in params:
            step, m, v = self._moments(p)
            w = self.state[p]["master_param"] if master else p
            by_step.setdefault(step, []).append((w, p.grad, m, v, p))
        out = []
        for step, ts in by_step.items():
            ws, grads, ms, vs, ps = map(list, zip(*ts))
            out.append((step, ws, grads, ms, vs, ps if master else None))
        return out
