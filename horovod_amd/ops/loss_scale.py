"""Loss scaling for the fused optimizers: the options, the scaler's state
and the per-step control values (see "Loss scaling" in docs/api.md).

The gradients of a scaled loss carry the scale S.  One norm pass over them
(csrc/clip_kernels.hip, scaled_clip_finalize_k) yields on the device

    found = 1 if the sum of squares is not finite, or an external flag is set
    norm  = sqrt(sum) / S                  # the unscaled global norm
    coef  = clip(norm) / S                 # clip = 1 without max_grad_norm

and updates the scale by the rule of torch._amp_update_scale_.  The step
kernels multiply each gradient by `coef` as they read it and return at once
when `found` is set, so nothing is unscaled in memory and the host does not
wait for the flag.  "Overflow" is a non-finite sum of squares: any inf or NaN
element, and also finite gradients whose norm passes about 1.8e19, which for
a loss scaler means the same thing, a scale that is too high.

Gradients the native pass does not take (CPU, sparse, several devices) get
the same values from torch ops.
"""
import torch

from horovod_amd import _core
from horovod_amd.ops import clip as _clip

DYNAMIC_DEFAULTS = dict(init_scale=2.0 ** 16, growth_factor=2.0,
                        backoff_factor=0.5, growth_interval=2000)


def check_loss_scale(loss_scale, loss_scale_args):
    """Validates the two options; -> the scaler's settings (DYNAMIC_DEFAULTS'
    keys) or None without loss scaling.  A static scale never changes:
    growth and backoff are 1."""
    if loss_scale is None:
        if loss_scale_args is not None:
            raise ValueError("loss_scale_args needs loss_scale='dynamic'")
        return None
    if loss_scale == "dynamic" and isinstance(loss_scale, str):
        args = dict(DYNAMIC_DEFAULTS)
        if loss_scale_args is not None:
            if not isinstance(loss_scale_args, dict) or \
                    set(loss_scale_args) - set(args):
                raise ValueError(
                    f"loss_scale_args takes {sorted(args)}, got "
                    f"{loss_scale_args!r}")
            args.update(loss_scale_args)
        interval = args["growth_interval"]
        if not (args["init_scale"] > 0 and args["growth_factor"] >= 1 and
                0 < args["backoff_factor"] <= 1 and
                isinstance(interval, int) and 1 <= interval < 2 ** 31):
            raise ValueError(
                "loss_scale_args needs init_scale > 0, growth_factor >= 1, "
                "0 < backoff_factor <= 1 and an integer growth_interval >= "
                f"1, got {loss_scale_args!r}")
        if float(args["init_scale"]) == float("inf"):
            raise ValueError("init_scale must be finite")
        return args
    if isinstance(loss_scale, (int, float)) and \
            not isinstance(loss_scale, bool) and \
            0 < loss_scale < float("inf"):
        if loss_scale_args is not None:
            raise ValueError("loss_scale_args needs loss_scale='dynamic'")
        return dict(init_scale=float(loss_scale), growth_factor=1.0,
                    backoff_factor=1.0, growth_interval=0)
    raise ValueError(
        "loss_scale must be None, 'dynamic' or a positive finite number, "
        f"got {loss_scale!r}")


def group_loss_scale(param_groups):
    """The scaler's settings all param groups agree on (None = no loss
    scaling): there is one scale for one loss.  Values set through a
    param-group dict are validated here like the constructor's."""
    values = [(g.get("loss_scale"), g.get("loss_scale_args"))
              for g in param_groups]
    settings = [check_loss_scale(*v) for v in values]
    if any(v != values[0] for v in values[1:]):
        raise ValueError(
            "loss_scale and loss_scale_args must be the same in every param "
            f"group (one loss has one scale), got {values}")
    return settings[0] if settings else None


class ScaledClip:
    """GradClip (clip.py) for gradients that carry a loss scale: unscaled
    `total_norm`, the coefficient `clip / scale`, and `found`, the overflow
    flag (fp32, 0 or 1).  All are 0-dim tensors on the device of the first
    gradient; nothing is read on the host here, except by the torch-op path
    when it updates a scale.

    scale, found_inf: 0-dim fp32 tensors or None; with `tracker` (0-dim
    int32) and `settings`, `scale` and `tracker` are updated in place.
    """

    def __init__(self, grads, max_norm, scale=None, found_inf=None,
                 tracker=None, settings=None):
        if max_norm is not None:
            max_norm = float(max_norm)
        # the kernel updates the scale where it lives
        if _clip.native_eligible(grads) and (
                tracker is None or scale.device == grads[0].device):
            device = grads[0].device
            update = {} if tracker is None else dict(
                growth_tracker=tracker,
                growth_factor=settings["growth_factor"],
                backoff_factor=settings["backoff_factor"],
                growth_interval=settings["growth_interval"])
            out = _core.multi_tensor_scaled_grad_norm(
                grads, max_norm,
                None if scale is None else scale.to(device),
                None if found_inf is None else found_inf.to(device),
                **update)
            self.total_norm, coef, self.found = out[0], out[1], out[2]
            # the 1-element views the step kernels take
            self._kernel = {device: (out[1:2], out[2:3])}
        else:
            device = grads[0].device if grads else (
                scale.device if scale is not None else torch.device("cpu"))
            raw = _clip.torch_norm(grads, fp32=True).to(device).float()
            inv = 1.0 / scale.to(device) if scale is not None else \
                torch.ones((), device=device)
            self.total_norm = raw * inv
            clip = torch.ones((), device=device) if max_norm is None else \
                torch.clamp(max_norm / (self.total_norm + 1e-6), max=1.0)
            coef = clip * inv
            found = ~torch.isfinite(raw)
            if found_inf is not None:
                found = found | (found_inf.to(device) != 0)
            self.found = found.float()
            self._kernel = {}
            if tracker is not None:
                _update_scale_(scale, tracker, bool(found), settings)
        self._values = {device: (coef, self.found)}

    def _on(self, device):
        v = self._values.get(device)
        if v is None:
            first = next(iter(self._values.values()))
            v = self._values[device] = tuple(t.to(device) for t in first)
        return v

    def coef(self, device):
        return self._on(device)[0]

    def scaled(self, g):
        """g * coef, out of place (0-dim coef: g keeps its dtype)."""
        return g * self.coef(g.device)

    def kernel_coef(self, device):
        return self._kernel_values(device)[0]

    def kernel_skip(self, device):
        return self._kernel_values(device)[1]

    def _kernel_values(self, device):
        k = self._kernel.get(device)
        if k is None:
            k = self._kernel[device] = tuple(
                t.float().reshape(1) for t in self._on(device))
        return k


class ExternalScale(ScaledClip):
    """The control values of a torch.amp.GradScaler step without clipping:
    no norm pass, coef = 1 / grad_scale, found = found_inf.  Either may be
    None."""

    def __init__(self, grads, grad_scale, found_inf):
        ref = grad_scale if grad_scale is not None else found_inf
        device = grads[0].device if grads else ref.device
        coef = torch.ones((), device=device) if grad_scale is None else \
            1.0 / grad_scale.to(device).float()
        self.found = torch.zeros((), device=device) if found_inf is None \
            else found_inf.to(device).float().reshape(())
        self.total_norm = None
        self._kernel = {}
        self._values = {device: (coef.reshape(()), self.found)}


def _update_scale_(scale, tracker, found, settings):
    """torch._amp_update_scale_'s rule, with the flag known on the host."""
    if found:
        scale.mul_(settings["backoff_factor"])
        tracker.zero_()
        return
    tracker.add_(1)
    if int(tracker) == settings["growth_interval"]:
        grown = scale * settings["growth_factor"]
        if bool(torch.isfinite(grown)):
            scale.copy_(grown)
        tracker.zero_()
