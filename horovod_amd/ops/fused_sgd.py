"""FusedSGD: SGD with momentum/weight-decay/update fused into one CDNA4
kernel launch over all parameter buckets (csrc/sgd_kernels.hip).

Torch-eager SGD issues 3-4 kernels per parameter (161 params x 4 = ~600
launches per ResNet-50 step); FusedSGD issues ceil(161/48) = 4.  Combine
with hvd.DistributedOptimizer exactly like torch.optim.SGD.

NOTE: the fused kernel path covers CUDA fp32 parameters with a dense
gradient and, with master_weights=True, CUDA fp16/bf16 parameters with a
dense gradient of their own dtype.  Other parameters (CPU, sparse gradients,
fp16/bf16 without master_weights) take a correct eager fallback and a
one-time warning is emitted so a benchmarked configuration cannot silently
lose the fusion.

master_weights=True keeps an fp32 `master_param` and an fp32
`momentum_buffer` for every fp16/bf16 parameter; the kernel updates the
master and writes it, rounded to nearest-even, into the parameter in the same
pass (see _fused_base.py).

max_grad_norm=<float> clips by the global L2 norm of all gradients inside
step(): one native multi-tensor norm pass (csrc/clip_kernels.hip), then the
step kernel multiplies each gradient by the coefficient as it reads it.
p.grad is left unscaled; the pre-clip norm is kept in `last_grad_norm`.

loss_scale="dynamic" (or a number for a static scale) makes the optimizer
its own loss scaler for fp16 training: backward runs on
`opt.scale_loss(loss)`; step() finds an overflow in one norm pass, unscales
inside the step kernel and skips the whole step on the device, without a
host read before the update (see _fused_base.py and loss_scale.py).
torch.amp.GradScaler.step(opt) is served by the same kernels.
"""
import torch

from horovod_amd import _core
from horovod_amd.ops._fused_base import FusedOptimizer


class FusedSGD(FusedOptimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0,
                 dampening=0.0, nesterov=False, max_grad_norm=None,
                 master_weights=False, loss_scale=None,
                 loss_scale_args=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("nesterov requires momentum > 0, dampening 0")
        super().__init__(params, dict(
            lr=lr, momentum=momentum, weight_decay=weight_decay,
            dampening=dampening, nesterov=nesterov,
            max_grad_norm=max_grad_norm, master_weights=master_weights,
            loss_scale=loss_scale, loss_scale_args=loss_scale_args))

    def _fused_update(self, params, group, coef, master, skip):
        momenta = []
        if group["momentum"] != 0:
            for p in params:
                st = self.state[p]
                if st.get("momentum_buffer") is None:
                    st["momentum_buffer"] = torch.zeros_like(
                        p, dtype=torch.float32)
                momenta.append(st["momentum_buffer"])
        ws = [self.state[p]["master_param"] for p in params] if master \
            else params
        _core.fused_sgd_step(ws, [p.grad for p in params], momenta,
                             group["lr"], group["momentum"],
                             group["weight_decay"], group["dampening"],
                             group["nesterov"], coef,
                             params if master else None, skip)

    def _eager_update(self, p, w, g, group):
        """w: the tensor to update (p, or its fp32 master); g: the dense,
        clipped gradient in w's dtype."""
        if group["weight_decay"]:
            g = g.add(w, alpha=group["weight_decay"])
        if group["momentum"]:
            st = self.state[p]
            buf = st.get("momentum_buffer")
            if buf is None:
                # in p's layout, so that a later step can take the kernel
                buf = st["momentum_buffer"] = torch.empty_like(w).copy_(g)
            else:
                buf.mul_(group["momentum"]).add_(g, alpha=1 - group["dampening"])
            g = g.add(buf, alpha=group["momentum"]) if group["nesterov"] else buf
        w.add_(g, alpha=-group["lr"])
