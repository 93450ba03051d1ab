"""Per-pass timing of the native SyncBatchNorm kernels (no allreduce in
between): stats, normalize (finalize + apply), backward reduce, backward
apply, each as the _core call a layer makes, timed with device events.

GB/s = activation bytes the pass reads + writes over the time of the whole
call (memset and small kernels included), so it is a lower bound on what
the big kernel alone reaches; small shapes are launch-bound.
ResNet-50 BN shapes at batch 64, bf16 and fp32, planar and channels_last.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from horovod_amd import _core

shapes = [(64,64,112,112),(64,256,56,56),(64,64,56,56),(64,512,28,28),
          (64,128,28,28),(64,1024,14,14),(64,256,14,14),(64,2048,7,7),
          (64,512,7,7)]
if os.environ.get("SBN_SHAPES"):  # e.g. SBN_SHAPES=64x64x112x112,64x256x56x56
    shapes = [tuple(int(v) for v in s.split("x"))
              for s in os.environ["SBN_SHAPES"].split(",")]
ITERS = int(os.environ.get("SBN_ITERS", "30"))
torch.cuda.set_device(0)


def timed(fn):
    for _ in range(5):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(ITERS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / ITERS * 1e3  # us per call


print("| shape | dtype | layout | stats us (GB/s) | normalize us (GB/s) | "
      "bwd reduce us (GB/s) | bwd apply us (GB/s) |")
print("|---|---|---|---|---|---|---|")
for dtype in (torch.bfloat16, torch.float32):
    for layout in ("planar", "channels_last"):
        for shp in shapes:
            x = torch.randn(*shp, device="cuda", dtype=dtype)
            if layout == "channels_last":
                x = x.contiguous(memory_format=torch.channels_last)
            dy = torch.randn_like(x)
            c = shp[1]
            w = torch.ones(c, device="cuda")
            b = torch.zeros(c, device="cuda")
            rm = torch.zeros(c, device="cuda")
            rv = torch.ones(c, device="cuda")
            nbytes = x.numel() * x.element_size()
            stats = _core.sync_bn_stats(x)
            y, mean, invstd = _core.sync_bn_normalize(x, stats, w, b, rm, rv,
                                                      0.1, 1e-5)
            sums = _core.sync_bn_backward_reduce(x, dy, mean, invstd)
            count = stats[2 * c:]
            passes = (
                (1, lambda: _core.sync_bn_stats(x)),
                (2, lambda: _core.sync_bn_normalize(x, stats, w, b, rm, rv,
                                                    0.1, 1e-5)),
                (2, lambda: _core.sync_bn_backward_reduce(x, dy, mean,
                                                          invstd)),
                (3, lambda: _core.sync_bn_backward_apply(x, dy, mean, invstd,
                                                         w, sums, count)),
            )
            cells = []
            for tensors, fn in passes:
                us = timed(fn)
                cells.append(f"{us:.1f} ({tensors * nbytes / us / 1e3:.0f})")
            dt = "bf16" if dtype == torch.bfloat16 else "fp32"
            print(f"| {'x'.join(map(str, shp))} | {dt} | {layout} | "
                  + " | ".join(cells) + " |", flush=True)
