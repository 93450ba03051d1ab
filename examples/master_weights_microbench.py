"""Microbench: one optimizer step on the parameter shapes of
horovod_amd.models.bert_large() held in bf16, one GPU, no clipping, for
FusedAdamW and FusedLAMB each:

  (a) master_weights=False: the eager per-parameter update a bf16 model
      takes without master weights (bf16 moments, ~8 launches a parameter)
  (b) master_weights=True: the master-weight kernels -- fp32 master and
      moments, bf16 gradient read and bf16 parameter written in the same pass
  (c) the fp32 kernels on fp32 parameters of the same element counts

(b) and (c) move the same bytes per element: 28 B for AdamW, 40 B for LAMB.

The three run in one process and alternate per repeat; each repeat is
MW_ITERS steps timed with device events after warm-up.  Spread is
(max - min) / median over the repeats: (b) vs (c) means something only
beyond the larger of their spreads.

  python examples/master_weights_microbench.py
  MW_ITERS=5 MW_REPEATS=3 python examples/master_weights_microbench.py
"""
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from horovod_amd.models import bert_large  # noqa: E402
from horovod_amd.ops import FusedAdamW, FusedLAMB  # noqa: E402

ITERS = int(os.environ.get("MW_ITERS", "10"))
REPEATS = int(os.environ.get("MW_REPEATS", "5"))
WARMUP = int(os.environ.get("MW_WARMUP", "3"))

with torch.device("meta"):
    shapes = [tuple(p.shape) for p in bert_large().parameters()]
numel = sum(torch.Size(s).numel() for s in shapes)
print(f"bert_large: {len(shapes)} tensors, {numel / 1e6:.1f} M elements",
      flush=True)

torch.cuda.set_device(0)

LR, B1, B2, WD = 1e-4, 0.9, 0.999, 0.01


def make_params(seed, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = []
    for s in shapes:
        p = (torch.randn(s, device="cuda", generator=g) * 0.02).to(dtype)
        p.requires_grad_(True)
        p.grad = torch.randn(s, device="cuda", generator=g).to(dtype)
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


def bench(cls, eps, bytes_per_element):
    name = cls.__name__
    kw = dict(lr=LR, betas=(B1, B2), eps=eps, weight_decay=WD)
    ps_a = make_params(1, torch.bfloat16)
    ps_b = make_params(1, torch.bfloat16)
    ps_c = make_params(1, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")        # (a) is the eager path
        opt_a = cls(ps_a, **kw)
    opt_b = cls(ps_b, master_weights=True, **kw)
    opt_c = cls(ps_c, **kw)
    paths = {f"{name} bf16, eager (master_weights=False)": opt_a.step,
             f"{name} bf16, master_weights=True": opt_b.step,
             f"{name} fp32": opt_c.step}
    times = {k: [] for k in paths}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fn in paths.values():
            timed(fn, WARMUP)
        for _ in range(REPEATS):
            for k, fn in paths.items():
                times[k].append(timed(fn, ITERS))
    # the parameter is the rounded master, or (b) measured something else
    assert all(torch.equal(p.detach(),
                           opt_b.state[p]["master_param"].bfloat16())
               for p in ps_b)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    print("| path | ms / step | spread |")
    print("|---|---|---|")
    for k in paths:
        print(f"| {k} | {med[k]:.3f} | {spread[k] * 100:.0f}% |")
    a, b, c = (med[k] for k in paths)
    tbs = bytes_per_element * numel / (b * 1e-3) / 1e12
    print(f"{name}: eager bf16 / master weights = {a / b:.2f}x, "
          f"master weights / fp32 fused = {b / c:.3f}x, master weights "
          f"{tbs:.2f} TB/s at {bytes_per_element} B per element", flush=True)
    return {"ms": med, "spread": spread, "repeats": times,
            "eager_over_master": a / b, "master_over_fp32": b / c,
            "master_tb_per_s": tbs}


results = {"FusedAdamW": bench(FusedAdamW, 1e-8, 28)}
torch.cuda.empty_cache()
results["FusedLAMB"] = bench(FusedLAMB, 1e-6, 40)
print(json.dumps({"tensors": len(shapes), "numel": numel, **results}))
