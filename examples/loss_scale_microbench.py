"""Microbench: loss scaling + AdamW step on the parameter shapes of
horovod_amd.models.bert_large(), fp32 gradients, one GPU.

  (a) scaler.unscale_(opt); found_inf.item(); FusedAdamW.step();
      scaler.update()
      -- the recipe without the option, i.e. what GradScaler.step() does
      for an optimizer that leaves the unscaling to it: an in-place unscale
      pass over all gradients, one host synchronisation on the flag, then
      the fused step (skipped on overflow)
  (b) FusedAdamW(loss_scale="dynamic").step()
      -- one native multi-tensor norm pass; unscale, skip and scale update
      on the device
  (c) (b) with max_grad_norm=1.0
  (d) FusedAdamW.step() without scaling, for scale

The four run in one process and alternate per repeat; each repeat is
LS_ITERS steps timed with device events after warm-up.  Spread is
(max - min) / median over the repeats: (a) vs (b) means something only
beyond (a)'s own spread.

step() of (b) waits for the overflow flag of the step before it (the host
runs at most one step ahead of the device).  To put a number on that, (b) is
also timed as a loop with that wait taken out (`lag-free`: the flag is
dropped, which is only sound here, where no step overflows), on the host
clock, which is where a stall shows.

  python examples/loss_scale_microbench.py
  LS_ITERS=5 LS_REPEATS=3 python examples/loss_scale_microbench.py
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from horovod_amd.models import bert_large  # noqa: E402
from horovod_amd.ops import FusedAdamW  # noqa: E402

ITERS = int(os.environ.get("LS_ITERS", "10"))
REPEATS = int(os.environ.get("LS_REPEATS", "5"))
WARMUP = int(os.environ.get("LS_WARMUP", "3"))
SCALE = 2.0 ** 10

with torch.device("meta"):
    shapes = [tuple(p.shape) for p in bert_large().parameters()]
numel = sum(torch.Size(s).numel() for s in shapes)
print(f"bert_large: {len(shapes)} tensors, {numel / 1e6:.1f} M elements",
      flush=True)

torch.cuda.set_device(0)


def make_params(seed, grad_scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = []
    for s in shapes:
        p = (torch.randn(s, device="cuda", generator=g) * 0.02)
        p.requires_grad_(True)
        p.grad = torch.randn(s, device="cuda", generator=g) * grad_scale
        ps.append(p)
    return ps


def timed(fn, n):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n  # ms per step


def host_timed(fn, n):
    """ms per step on the host clock, device drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


kw = dict(lr=1e-4, weight_decay=0.01)
# a static scale keeps the gradients of every step at the scale they carry
scaling = dict(loss_scale=SCALE)
ps_a = make_params(1, SCALE)
ps_b, ps_c = make_params(1, SCALE), make_params(1, SCALE)
ps_d = make_params(1, 1.0)
opt_a = FusedAdamW(ps_a, **kw)
opt_b = FusedAdamW(ps_b, **scaling, **kw)
opt_c = FusedAdamW(ps_c, max_grad_norm=1.0, **scaling, **kw)
opt_d = FusedAdamW(ps_d, **kw)
scaler = torch.amp.GradScaler("cuda", init_scale=SCALE,
                              growth_interval=10 ** 9)
scaler.scale(torch.ones((), device="cuda"))      # makes the scale tensor
grads_a = [p.grad for p in ps_a]
scaled_a = [g.clone() for g in grads_a]


def step_a():
    # backward would leave scaled gradients; unscale_ works in place, so
    # put them back first (outside the recipe, but inside the timing: (a)
    # is charged one foreach copy per step, noted in docs/benchmarks.md)
    torch._foreach_copy_(grads_a, scaled_a)
    scaler.unscale_(opt_a)
    found = scaler._per_optimizer_states[id(opt_a)]["found_inf_per_device"]
    if not sum(v.item() for v in found.values()):
        opt_a.step()
    scaler.update()


def restore_a():
    torch._foreach_copy_(grads_a, scaled_a)


def step_b_lag_free():
    opt_b._pending = None
    opt_b.step()


paths = {"unscale_ + item() + step": step_a,
         "restore gradients only": restore_a,
         "loss_scale step": opt_b.step,
         "loss_scale + clip step": opt_c.step,
         "step, no scaling": opt_d.step}
times = {k: [] for k in paths}
for fn in paths.values():
    timed(fn, WARMUP)
for _ in range(REPEATS):
    for k, fn in paths.items():
        times[k].append(timed(fn, ITERS))

host = {"loss_scale step": opt_b.step, "lag-free": step_b_lag_free}
host_times = {k: [] for k in host}
for _ in range(REPEATS):
    for k, fn in host.items():
        host_times[k].append(host_timed(fn, ITERS))
assert opt_b.get_loss_scale() == SCALE and opt_b.skipped_steps == 0

med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print("| path | ms / step | spread |")
print("|---|---|---|")
for k in paths:
    print(f"| {k} | {med[k]:.3f} | {spread[k] * 100:.0f}% |")
a = med["unscale_ + item() + step"] - med["restore gradients only"]
b = med["loss_scale step"]
print(f"(a) net of the restore = {a:.3f} ms; (a) / (b) = {a / b:.2f}x")
host_med = {k: statistics.median(v) for k, v in host_times.items()}
host_spread = {k: (max(v) - min(v)) / host_med[k]
               for k, v in host_times.items()}
print("| loop of (b), host clock | ms / step | spread |")
print("|---|---|---|")
for k in host:
    print(f"| {k} | {host_med[k]:.3f} | {host_spread[k] * 100:.0f}% |")
print(json.dumps({"tensors": len(shapes), "numel": numel, "ms": med,
                  "spread": spread, "repeats": times, "host_ms": host_med,
                  "host_spread": host_spread, "host_repeats": host_times}))
