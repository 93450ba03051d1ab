"""Microbench: global-norm clipping + AdamW step on the parameter shapes of
horovod_amd.models.bert_large(), fp32 gradients, one GPU.

  (a) torch.nn.utils.clip_grad_norm_(params, 1.0); FusedAdamW.step()
      -- the recipe without the option: a foreach norm pass, a handful of
      scalar kernels, an in-place scale pass, then the fused step
  (b) FusedAdamW(max_grad_norm=1.0).step()
      -- one native multi-tensor norm pass, coefficient applied inside the
      step kernel
  (c) FusedAdamW.step() without clipping, for scale

The three run in one process and alternate per repeat; each repeat is
CLIP_ITERS steps timed with device events after warm-up.  Spread is
(max - min) / median over the repeats: (a) vs (b) means something only
beyond (a)'s own spread.

  python examples/clip_microbench.py
  CLIP_ITERS=5 CLIP_REPEATS=3 python examples/clip_microbench.py
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from horovod_amd.models import bert_large  # noqa: E402
from horovod_amd.ops import FusedAdamW  # noqa: E402

ITERS = int(os.environ.get("CLIP_ITERS", "10"))
REPEATS = int(os.environ.get("CLIP_REPEATS", "5"))
WARMUP = int(os.environ.get("CLIP_WARMUP", "3"))

with torch.device("meta"):
    shapes = [tuple(p.shape) for p in bert_large().parameters()]
numel = sum(torch.Size(s).numel() for s in shapes)
print(f"bert_large: {len(shapes)} tensors, {numel / 1e6:.1f} M elements",
      flush=True)

torch.cuda.set_device(0)


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


kw = dict(lr=1e-4, weight_decay=0.01)
ps_a, ps_b, ps_c = make_params(1), make_params(1), make_params(1)
opt_a = FusedAdamW(ps_a, **kw)
opt_b = FusedAdamW(ps_b, max_grad_norm=1.0, **kw)
opt_c = FusedAdamW(ps_c, **kw)


def step_a():
    torch.nn.utils.clip_grad_norm_(ps_a, 1.0)
    opt_a.step()


paths = {"torch clip + step": step_a, "fused clip step": opt_b.step,
         "step, no clip": opt_c.step}
times = {k: [] for k in paths}
for fn in paths.values():
    timed(fn, WARMUP)
for _ in range(REPEATS):
    for k, fn in paths.items():
        times[k].append(timed(fn, ITERS))

med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print("| path | ms / step | spread |")
print("|---|---|---|")
for k in paths:
    print(f"| {k} | {med[k]:.3f} | {spread[k] * 100:.0f}% |")
a, b = med["torch clip + step"], med["fused clip step"]
print(f"torch clip + step / fused clip step = {a / b:.2f}x")
print(json.dumps({"tensors": len(shapes), "numel": numel,
                  "ms": med, "spread": spread, "repeats": times}))
