"""Scaffold shared by FusedSGD, FusedAdamW, FusedLAMB and FusedLARS.

FusedOptimizer owns the max_grad_norm, master_weights and loss_scale options,
`last_grad_norm`, the group defaults a foreign state dict may lack, and the
step() skeleton: closure, one GradClip (or, with a loss scale, ScaledClip)
over all groups, then per group the split into parameters the kernels take
and parameters that take the eager update, with a one-time warning so a
benchmarked configuration cannot silently lose the fusion.  The kernels take
CUDA fp32 parameters with a dense gradient of their own layout and, in a
master_weights group, CUDA fp16/bf16 parameters with such a gradient of their
own dtype.

master_weights=True gives every fp16/bf16 parameter of the group fp32 state:
`master_param`, made from p.float() when the parameter first has a gradient,
and fp32 moments.  The update runs on the master in fp32 and the parameter
is overwritten with the rounded master, so the master is authoritative: a
parameter changed from outside is not picked up.  fp32 parameters of the
group are updated as ever and get no master.

loss_scale="dynamic" (or a positive number for a static scale) makes the
optimizer its own loss scaler: backward runs on `opt.scale_loss(loss)`, and
step() unscales the gradients as the kernels read them, skips the whole step
on the device when they overflowed, and updates the scale there (see
loss_scale.py).  The host launches such a step without knowing whether it
will be skipped.  It learns of it one step() later, from a flag copied to
pinned memory: bias correction is folded on the host from the integer
`step`, so the next step(), state_dict() or get_loss_scale() first waits for
that flag and, if it was set, takes back the `step` increments of the
skipped step.  The host thus runs at most one step() ahead of the device.
A torch.amp.GradScaler is served by the same kernels: step() honours the
`grad_scale` and `found_inf` attributes the scaler sets.

A subclass supplies `_eager_update(p, w, g, group)` and `_fused_update(params,
group, coef, master, skip)`, its `_core.fused_*` call.  Every option stays in
`param_groups`: hvd.DistributedOptimizer rebuilds the optimizer from those
alone (the rebuilt optimizer starts from init_scale: wrap before training, or
load a state dict afterwards).
"""
import itertools
import warnings

import torch

from horovod_amd.ops import clip as _clip
from horovod_amd.ops import loss_scale as _ls

_LOW_PRECISION = (torch.float16, torch.bfloat16)
# state that is fp32 for a master-weight parameter, whatever its own dtype
_MASTER_STATE_KEYS = ("master_param", "exp_avg", "exp_avg_sq",
                      "momentum_buffer")


def _fp32_like(p):
    """fp32 zeros in p's layout."""
    return torch.zeros_like(p, dtype=torch.float32)


class FusedOptimizer(torch.optim.Optimizer):
    # group keys a loaded state dict (e.g. torch.optim.AdamW's) may lack
    _GROUP_DEFAULTS = {"max_grad_norm": None, "master_weights": False,
                       "loss_scale": None, "loss_scale_args": None}
    # torch.amp.GradScaler.step() then leaves unscaling and the skip to
    # step(), which finds them in self.grad_scale and self.found_inf
    _step_supports_amp_scaling = True

    def __init__(self, params, defaults):
        _clip.check_max_grad_norm(defaults["max_grad_norm"])
        _ls.check_loss_scale(defaults["loss_scale"],
                             defaults["loss_scale_args"])
        super().__init__(params, defaults)
        for group in self.param_groups:   # values given per param group
            _clip.check_max_grad_norm(group["max_grad_norm"])
            _ls.check_loss_scale(group["loss_scale"],
                                 group["loss_scale_args"])
        self.last_grad_norm = None
        # loss scaling: the overflow flag of the last scaled step (device),
        # the settled number of skipped steps, the scaler's device state
        # (made on first use) and the flag of a step the host has not yet
        # heard of: (flag on the host, event or None, the step's parameters)
        self.last_found_inf = None
        self.skipped_steps = 0
        self._scale = self._growth_tracker = None
        self._pending = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for key, value in self._GROUP_DEFAULTS.items():
                group.setdefault(key, value)
        # an unpickled optimizer has not been through __init__
        for name, value in (("last_found_inf", None), ("skipped_steps", 0),
                            ("_scale", None), ("_growth_tracker", None),
                            ("_pending", None)):
            self.__dict__.setdefault(name, value)

    # ---- loss scaling ------------------------------------------------------

    def _scaler_settings(self):
        """The first group's loss-scale settings (None: no loss scaling);
        step() insists that all groups agree."""
        for group in self.param_groups:
            return _ls.check_loss_scale(group.get("loss_scale"),
                                        group.get("loss_scale_args"))
        return None

    def _scaler_state(self, settings):
        """-> the scale (0-dim fp32) and the growth tracker (0-dim int32),
        made on the device of the first parameter when first asked for."""
        if self._scale is None:
            device = self.param_groups[0]["params"][0].device
            self._scale = torch.full((), settings["init_scale"],
                                     dtype=torch.float32, device=device)
            self._growth_tracker = torch.zeros((), dtype=torch.int32,
                                               device=device)
        return self._scale, self._growth_tracker

    @property
    def loss_scale_tensor(self):
        """The current scale, a 0-dim fp32 device tensor updated in place by
        step() (None without loss scaling)."""
        settings = self._scaler_settings()
        return None if settings is None else self._scaler_state(settings)[0]

    def scale_loss(self, loss):
        """loss * scale: a device multiply, no synchronisation."""
        scale = self.loss_scale_tensor
        if scale is None:
            raise RuntimeError(
                f"{type(self).__name__}.scale_loss needs the loss_scale "
                "option")
        return loss * scale.to(loss.device)

    def get_loss_scale(self):
        """The current scale as a float; waits for the device."""
        self._settle()
        scale = self.loss_scale_tensor
        return None if scale is None else float(scale)

    def _settle(self):
        """Waits for the overflow flag of the last scaled step and, if that
        step was skipped on the device, takes back its `step` counts."""
        if self._pending is None:
            return
        flag, event, params = self._pending
        self._pending = None
        if event is not None:
            event.synchronize()
        if float(flag) != 0:
            self.skipped_steps += 1
            for p in params:
                if "step" in self.state[p]:
                    self.state[p]["step"] -= 1

    def _track(self, control, params):
        """Right behind the norm pass of a scaled step, before the update is
        launched: start the copy of its flag for _settle, which then waits
        for the norm pass alone.  `params`: the parameters of the step."""
        self.last_found_inf = found = control.found
        flag, event = found, None
        if found.is_cuda:
            flag = torch.empty((), dtype=torch.float32, pin_memory=True)
            flag.copy_(found, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(found.device))
        self._pending = (flag, event, params)

    def _step_control(self, grads, max_grad_norm):
        """-> what scales the gradients of this step and may skip it: a
        GradClip, a ScaledClip, or None."""
        settings = _ls.group_loss_scale(self.param_groups)
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        if grad_scale is not None or found_inf is not None:
            if settings is not None:
                raise RuntimeError(
                    f"{type(self).__name__}: a torch.amp.GradScaler and the "
                    "loss_scale option both want to scale the loss; use one")
            if max_grad_norm is None:
                return _ls.ExternalScale(grads, grad_scale, found_inf)
            return _ls.ScaledClip(grads, max_grad_norm, grad_scale, found_inf)
        if settings is not None:
            scale, tracker = self._scaler_state(settings)
            if settings["growth_interval"] == 0:   # static: never updated
                tracker = None
            return _ls.ScaledClip(grads, max_grad_norm, scale, None, tracker,
                                  settings)
        if max_grad_norm is not None:
            return _clip.GradClip(grads, max_grad_norm)
        return None

    def state_dict(self):
        """With loss scaling, torch's dict and a top-level "loss_scaler":
        {"scale": float, "growth_tracker": int}."""
        self._settle()
        sd = super().state_dict()
        settings = self._scaler_settings()
        if settings is not None:
            scale, tracker = self._scaler_state(settings)
            sd["loss_scaler"] = {"scale": float(scale),
                                 "growth_tracker": int(tracker)}
        return sd

    def _load_loss_scaler(self, saved):
        settings = self._scaler_settings()
        if saved is None or settings is None:
            return
        scale, tracker = self._scaler_state(settings)
        scale.fill_(float(saved["scale"]))
        tracker.fill_(int(saved["growth_tracker"]))

    def load_state_dict(self, state_dict):
        """torch casts every floating state tensor to its parameter's dtype;
        the fp32 state of master-weight parameters is restored from the
        given dict instead, on the parameter's device.  A "loss_scaler"
        entry restores scale and tracker; without one they stay."""
        self._settle()
        super().load_state_dict(state_dict)
        self._load_loss_scaler(state_dict.get("loss_scaler"))
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
        self._settle()
        max_grad_norm = _clip.group_max_grad_norm(self.param_groups)
        with_grad = [p for group in self.param_groups
                     for p in group["params"] if p.grad is not None]
        clip = self._step_control([p.grad for p in with_grad], max_grad_norm)
        if clip is not None and clip.total_norm is not None:
            self.last_grad_norm = clip.total_norm
        # a scaled step: the kernels skip on the device flag; the eager
        # update reads it on the host
        scaled = isinstance(clip, _ls.ScaledClip)
        if scaled:
            self._track(clip, with_grad)
        eager_skip = None
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
                if scaled and eager_skip is None:
                    eager_skip = bool(clip.found)
                if eager_skip:
                    continue
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
                        master,
                        clip.kernel_skip(params[0].device) if scaled
                        else None)
        if scaled and not clip.found.is_cuda:
            self._settle()      # the flag is on the host already
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
