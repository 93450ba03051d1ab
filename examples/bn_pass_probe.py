"""Per-pass timing of the fused BatchNorm(+Add)+ReLU kernels: stats, apply,
backward stats and backward apply, each as _core.fused_bn_pass issues it
(the reductions with their memset), timed with device events.

GB/s = activation bytes the pass reads + writes over the time of the whole
call, so it is a lower bound on what the big kernel alone reaches; small
shapes are launch-bound.  ResNet-50 BN shapes at batch 64, bf16,
channels_last.  "add" rows are the FusedBNAddReLU variant: its backward
stats also write g = dy * (y > 0), and its backward apply reads g and x.
The two "no y" columns are the backward passes of a layer without a residual
as the modules issue them: the ReLU mask is recomputed from x, so y is not
read (2 and 3 tensors moved instead of 3 and 4).
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from horovod_amd import _core

shapes = [(64,64,112,112),(64,256,56,56),(64,64,56,56),(64,512,28,28),
          (64,128,28,28),(64,1024,14,14),(64,256,14,14),(64,2048,7,7),
          (64,512,7,7)]
if os.environ.get("BN_SHAPES"):  # e.g. BN_SHAPES=64x64x112x112,64x256x56x56
    shapes = [tuple(int(v) for v in s.split("x"))
              for s in os.environ["BN_SHAPES"].split(",")]
ITERS = int(os.environ.get("BN_ITERS", "30"))
# BN_PROBE_FROM_G=0: time the add variant's backward apply as reading x, y
# and dy (what it did before it read the stored g)
FROM_G = os.environ.get("BN_PROBE_FROM_G", "1") != "0"
dtype = torch.bfloat16
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


print("| shape | variant | stats us (GB/s) | apply us (GB/s) | "
      "bwd stats us (GB/s) | bwd apply us (GB/s) | "
      "bwd stats, no y us (GB/s) | bwd apply, no y us (GB/s) |")
print("|---|---|---|---|---|---|---|---|")
for shp in shapes:
    def cl():
        return torch.randn(*shp, device="cuda", dtype=dtype).contiguous(
            memory_format=torch.channels_last)
    x, res, dy = cl(), cl(), cl()
    y = torch.relu(cl())
    out = torch.empty_like(x)
    c = shp[1]
    mean = torch.zeros(c, device="cuda")
    invstd = torch.ones(c, device="cuda")
    w = torch.ones(c, device="cuda")
    b = torch.zeros(c, device="cuda")
    nbytes = x.numel() * x.element_size()

    def p(which, a_, b_, out_):
        return lambda: _core.fused_bn_pass(which, x, a_, b_, out_, mean,
                                           invstd, w, b)
    for variant in ("relu", "add"):
        add = variant == "add"
        passes = (
            (1, p(0, None, None, None)),
            (3 if add else 2, p(1, res if add else None, None, out)),
            (4 if add else 3, p(2, y, dy, out if add else None)),
            ((3 if FROM_G else 4) if add else 4,
             p(3, None if (add and FROM_G) else y, dy, out)),
        )
        if not add:
            passes += ((2, p(4, None, dy, None)), (3, p(5, None, dy, out)))
        cells = []
        for tensors, fn in passes:
            us = timed(fn)
            cells.append(f"{us:.1f} ({tensors * nbytes / us / 1e3:.0f})")
        cells += ["-"] * (6 - len(cells))
        print(f"| {'x'.join(map(str, shp))} | {variant} | "
              + " | ".join(cells) + " |", flush=True)
