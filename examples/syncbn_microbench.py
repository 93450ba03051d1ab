"""Per-shape microbench: native SyncBatchNorm path vs the composite ATen
path (HOROVOD_SYNC_BN_NATIVE=0), training fwd+bwd of _SyncBatchNormFn at
np=1, ResNet-50 BN shapes at batch 64, bf16 and fp32, planar and
channels_last.

Both paths run in one process and alternate per repeat; each repeat is
SBN_ITERS fwd+bwd calls timed with device events.  The spread columns are
(max - min) / median over the repeats of each path: a ratio is only
meaningful beyond the composite path's own spread.

  python examples/syncbn_microbench.py            # full table
  SBN_SHAPES=64x64x56x56 SBN_REPEATS=3 python examples/syncbn_microbench.py
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics
import torch
import horovod_amd.torch as hvd
from horovod_amd.torch.sync_batch_norm import _SyncBatchNormFn, native_eligible

shapes = [(64,64,112,112),(64,256,56,56),(64,64,56,56),(64,512,28,28),
          (64,128,28,28),(64,1024,14,14),(64,256,14,14),(64,2048,7,7),
          (64,512,7,7)]
if os.environ.get("SBN_SHAPES"):  # e.g. SBN_SHAPES=64x64x112x112,64x256x56x56
    shapes = [tuple(int(v) for v in s.split("x"))
              for s in os.environ["SBN_SHAPES"].split(",")]
ITERS = int(os.environ.get("SBN_ITERS", "20"))
REPEATS = int(os.environ.get("SBN_REPEATS", "5"))
WARMUP = int(os.environ.get("SBN_WARMUP", "5"))

hvd.init()
torch.cuda.set_device(0)


def set_path(native):
    os.environ["HOROVOD_SYNC_BN_NATIVE"] = "1" if native else "0"


def timed(fn, n):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n  # ms per fwd+bwd


print("| shape | dtype | layout | native ms | composite ms | "
      "composite/native | native spread | composite spread |")
print("|---|---|---|---|---|---|---|---|")
for dtype in (torch.bfloat16, torch.float32):
    for layout in ("planar", "channels_last"):
        for (n, c, h, w) in shapes:
            x = torch.randn(n, c, h, w, device="cuda", dtype=dtype)
            if layout == "channels_last":
                x = x.contiguous(memory_format=torch.channels_last)
            x.requires_grad_(True)
            dy = torch.randn_like(x)
            # module-style parameters: fp32 weights and running stats
            wt = torch.ones(c, device="cuda", requires_grad=True)
            bs = torch.zeros(c, device="cuda", requires_grad=True)
            rm = torch.zeros(c, device="cuda")
            rv = torch.ones(c, device="cuda")

            def step():
                y = _SyncBatchNormFn.apply(x, wt, bs, rm, rv, 1e-5, 0.1,
                                           hvd.global_process_set)
                y.backward(dy)
                x.grad = wt.grad = bs.grad = None

            times = {True: [], False: []}
            for native in (True, False):
                set_path(native)
                assert native_eligible(x) == native
                timed(step, WARMUP)
            for _ in range(REPEATS):
                for native in (True, False):
                    set_path(native)
                    times[native].append(timed(step, ITERS))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
            dt = "bf16" if dtype == torch.bfloat16 else "fp32"
            print(f"| {n}x{c}x{h}x{w} | {dt} | {layout} | {med[True]:.3f} | "
                  f"{med[False]:.3f} | {med[False] / med[True]:.2f}x | "
                  f"{spread[True] * 100:.0f}% | {spread[False] * 100:.0f}% |",
                  flush=True)
            del x, dy
hvd.shutdown()
