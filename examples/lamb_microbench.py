"""Microbench: one LAMB step on the parameter shapes of
horovod_amd.models.bert_large(), fp32, one GPU, no clipping.

  (a) eager LAMB written here with torch._foreach_* ops and one
      torch.linalg.vector_norm per tensor for each of the two norms
  (b) FusedLAMB.step()
      -- three native launches per 48 tensors (csrc/lamb_kernels.hip)
  (c) FusedAdamW.step(), for scale: LAMB moves 40 B per element, AdamW 28 B

The three run in one process and alternate per repeat; each repeat is
LAMB_ITERS steps timed with device events after warm-up.  Spread is
(max - min) / median over the repeats: (a) vs (b) means something only
beyond the larger of their spreads.

  python examples/lamb_microbench.py
  LAMB_ITERS=5 LAMB_REPEATS=3 python examples/lamb_microbench.py
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from horovod_amd.models import bert_large  # noqa: E402
from horovod_amd.ops import FusedAdamW, FusedLAMB  # noqa: E402

ITERS = int(os.environ.get("LAMB_ITERS", "10"))
REPEATS = int(os.environ.get("LAMB_REPEATS", "5"))
WARMUP = int(os.environ.get("LAMB_WARMUP", "3"))

with torch.device("meta"):
    shapes = [tuple(p.shape) for p in bert_large().parameters()]
numel = sum(torch.Size(s).numel() for s in shapes)
print(f"bert_large: {len(shapes)} tensors, {numel / 1e6:.1f} M elements",
      flush=True)

torch.cuda.set_device(0)

LR, B1, B2, EPS, WD = 1e-4, 0.9, 0.999, 1e-6, 0.01


def make_params(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = []
    for s in shapes:
        p = (torch.randn(s, device="cuda", generator=g) * 0.02)
        p.requires_grad_(True)
        p.grad = torch.randn(s, device="cuda", generator=g)
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


class EagerLamb:
    """The definition of docs/api.md in foreach ops, no host reads."""

    def __init__(self, params):
        self.ps = [p.detach() for p in params]
        self.gs = [p.grad for p in params]
        self.ms = [torch.zeros_like(p) for p in self.ps]
        self.vs = [torch.zeros_like(p) for p in self.ps]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        torch._foreach_mul_(self.ms, B1)
        torch._foreach_add_(self.ms, self.gs, alpha=1 - B1)
        torch._foreach_mul_(self.vs, B2)
        torch._foreach_addcmul_(self.vs, self.gs, self.gs, value=1 - B2)
        us = torch._foreach_div(self.vs, 1 - B2 ** self.t)
        torch._foreach_sqrt_(us)
        torch._foreach_add_(us, EPS)
        torch._foreach_reciprocal_(us)
        torch._foreach_mul_(us, self.ms)
        torch._foreach_div_(us, 1 - B1 ** self.t)
        torch._foreach_add_(us, self.ps, alpha=WD)
        w_norms = [torch.linalg.vector_norm(p) for p in self.ps]
        u_norms = [torch.linalg.vector_norm(u) for u in us]
        w, u = torch.stack(w_norms), torch.stack(u_norms)
        trust = torch.where((w > 0) & (u > 0), w / u, torch.ones_like(w))
        torch._foreach_mul_(us, list((trust * -LR).unbind()))
        torch._foreach_add_(self.ps, us)


ps_a, ps_b, ps_c = make_params(1), make_params(1), make_params(1)
opt_a = EagerLamb(ps_a)
opt_b = FusedLAMB(ps_b, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
opt_c = FusedAdamW(ps_c, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)

paths = {"eager foreach LAMB": opt_a.step, "FusedLAMB step": opt_b.step,
         "FusedAdamW step": opt_c.step}
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
print("| path | ms / step | spread |")
print("|---|---|---|")
for k in paths:
    print(f"| {k} | {med[k]:.3f} | {spread[k] * 100:.0f}% |")
a, b, c = (med[k] for k in paths)
print(f"eager / fused = {a / b:.2f}x, FusedLAMB / FusedAdamW = {b / c:.2f}x")
print(f"FusedLAMB: {40 * numel / (b * 1e-3) / 1e12:.2f} TB/s "
      "at 40 B per element")
print(json.dumps({"tensors": len(shapes), "numel": numel,
                  "ms": med, "spread": spread, "repeats": times,
                  "max_abs_dev": dev}))
