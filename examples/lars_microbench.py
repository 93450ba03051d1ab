"""Microbench: one LARS step on the 161 parameter tensors of
horovod_amd.models.resnet50(), fp32, one GPU, no clipping.

  (a) eager LARS written here with torch._foreach_* ops and
      torch._foreach_norm for the two norms per tensor, no host reads
  (b) FusedLARS.step()
      -- three native launches per 48 tensors (csrc/lars_kernels.hip)
  (c) FusedSGD.step(), for scale: LARS moves 28 B per element, SGD 20 B

All three use one weight decay for every tensor, so every tensor takes the
adaptive branch.  They run in one process and alternate per repeat; each
repeat is LARS_ITERS steps timed with device events after warm-up.  Spread is
(max - min) / median over the repeats: a difference between two paths means
something only beyond the larger of their spreads.  The bytes/s figure is the
28 B per element over the step time (host launches included), a lower bound
on what the kernels reach.

  python examples/lars_microbench.py
  LARS_ITERS=50 LARS_REPEATS=3 python examples/lars_microbench.py
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from horovod_amd.models import resnet50  # noqa: E402
from horovod_amd.ops import FusedLARS, FusedSGD  # noqa: E402

ITERS = int(os.environ.get("LARS_ITERS", "100"))
REPEATS = int(os.environ.get("LARS_REPEATS", "5"))
WARMUP = int(os.environ.get("LARS_WARMUP", "10"))

with torch.device("meta"):
    shapes = [tuple(p.shape) for p in resnet50().parameters()]
numel = sum(torch.Size(s).numel() for s in shapes)
chunks = sum(-(-torch.Size(s).numel() // 8192) for s in shapes)
batches = -(-len(shapes) // 48)
print(f"resnet50: {len(shapes)} tensors, {numel / 1e6:.1f} M elements, "
      f"{chunks} chunks", flush=True)

torch.cuda.set_device(0)

LR, MU, WD, TC, EPS = 0.1, 0.9, 5e-5, 0.001, 1e-8


def make_params(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = []
    for s in shapes:
        p = (torch.randn(s, device="cuda", generator=g) * 0.05)
        p.requires_grad_(True)
        p.grad = torch.randn(s, device="cuda", generator=g) * 0.01
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


class EagerLars:
    """The definition of docs/api.md in foreach ops, no host reads."""

    def __init__(self, params):
        self.ps = [p.detach() for p in params]
        self.gs = [p.grad for p in params]
        self.ms = [torch.zeros_like(p) for p in self.ps]

    @torch.no_grad()
    def step(self):
        w = torch.stack(torch._foreach_norm(self.ps))
        g = torch.stack(torch._foreach_norm(self.gs))
        trust = torch.where((w > 0) & (g > 0), TC * w / (g + WD * w + EPS),
                            torch.ones_like(w))
        ds = torch._foreach_add(self.gs, self.ps, alpha=WD)
        torch._foreach_mul_(ds, list(trust.unbind()))
        torch._foreach_mul_(self.ms, MU)
        torch._foreach_add_(self.ms, ds)
        torch._foreach_add_(self.ps, self.ms, alpha=-LR)


ps_a, ps_b, ps_c = make_params(1), make_params(1), make_params(1)
opt_a = EagerLars(ps_a)
opt_b = FusedLARS(ps_b, lr=LR, momentum=MU, weight_decay=WD,
                  trust_coefficient=TC, eps=EPS)
opt_c = FusedSGD(ps_c, lr=LR, momentum=MU, weight_decay=WD)

paths = {"eager foreach LARS": opt_a.step, "FusedLARS step": opt_b.step,
         "FusedSGD step": opt_c.step}
launches = {"eager foreach LARS": "not counted",
            "FusedLARS step": 3 * batches, "FusedSGD step": batches}
times = {k: [] for k in paths}
for fn in paths.values():
    timed(fn, WARMUP)
# same trajectory, or the comparison is of two different things
dev = max((p.detach() - q.detach()).abs().max().item()
          for p, q in zip(ps_a, ps_b))
print(f"max |eager - fused| over all parameters after warm-up: {dev:.3e}")
for _ in range(REPEATS):
    for k, fn in paths.items():
        times[k].append(timed(fn, ITERS))

med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print("| path | ms / step | spread | native launches / step |")
print("|---|---|---|---|")
for k in paths:
    print(f"| {k} | {med[k]:.3f} | {spread[k] * 100:.0f}% | {launches[k]} |")
a, b, c = (med[k] for k in paths)
print(f"eager / fused = {a / b:.2f}x, FusedLARS / FusedSGD = {b / c:.2f}x")
print(f"FusedLARS: {28 * numel / (b * 1e-3) / 1e12:.3f} TB/s "
      "at 28 B per element over the step time")
print(json.dumps({"tensors": len(shapes), "numel": numel, "chunks": chunks,
                  "ms": med, "spread": spread, "repeats": times,
                  "launches": launches, "max_abs_dev": dev}))
