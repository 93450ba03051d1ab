"""Per-pass microbench: FusedDropoutAddLayerNorm against the composite
F.layer_norm(residual + F.dropout(x)) in the same dtype (bf16, training),
forward and backward timed apart with device events.

For each pass it prints the bytes the pass has to move, computed from the
shapes, the time between the device events, the host's time to issue the
pass, and bytes over the event time.  That quotient is an end-to-end rate of
the pass (launches and allocator included, not a kernel's share of peak), and
only where the row is marked "device": in a row marked "host" the device
waited for the host, and the time is the host's.  Kernel times come from a
kernel trace of this script, one configuration per process (LN_SHAPES, LN_PS,
LN_PATHS below).  With E = M * H elements of s bytes:
  forward   reads x and the residual, writes y and z (z only when it is not
            x: here always, there is a residual): 4 * E * s, plus the 2 * M
            fp32 statistics
  backward  reads dy and z, writes dz, and dx when p > 0: (3 or 4) * E * s,
            plus reading the statistics and writing 2 * H fp32 gradients
Needs a GPU: a measurement without one would say nothing.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from horovod_amd.ops import FusedDropoutAddLayerNorm  # noqa: E402

SHAPES = [(1024, 1024), (8192, 1024), (16384, 1024), (8192, 768)]
PS = [0.0, 0.1]
PATHS = ["fused", "composite"]
# one configuration per process for a kernel trace, e.g.
# LN_SHAPES=8192x1024 LN_PS=0.1 LN_PATHS=fused
if os.environ.get("LN_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["LN_SHAPES"].split(",")]
if os.environ.get("LN_PS"):
    PS = [float(v) for v in os.environ["LN_PS"].split(",")]
if os.environ.get("LN_PATHS"):
    PATHS = os.environ["LN_PATHS"].split(",")
DTYPE = torch.bfloat16
ITERS = int(os.environ.get("LN_ITERS", "50"))
WARMUP = 10


def pass_bytes(M, H, p, s):
    E = M * H
    fwd = 4 * E * s + 2 * M * 4
    bwd = (4 if p > 0 else 3) * E * s + 2 * M * 4 + 2 * H * 4
    return fwd, bwd


def time_passes(fn, x, res, dy):
    """Mean ms of the forward and of the backward over ITERS runs: between
    device events, and on the host clock around issuing the pass (no
    synchronise inside the window)."""
    events, host = [], [0.0, 0.0]
    for it in range(WARMUP + ITERS):
        if it == WARMUP:
            torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        t0 = time.perf_counter()
        y = fn(x, res)
        t1 = time.perf_counter()
        e[1].record()
        y.backward(dy)
        t2 = time.perf_counter()
        e[2].record()
        x.grad = res.grad = None
        if it >= WARMUP:
            events.append(e)
            host[0] += t1 - t0
            host[1] += t2 - t1
    # One synchronise for the whole window.  The events bracket device work
    # only while the host issues a pass faster than the device runs it; when
    # the host is the slower one the device idles between launches and the
    # event interval is the host's issue time.  The caller compares the two
    # and marks such rows: their MB / ms is not a bandwidth.
    torch.cuda.synchronize()
    dev = (sum(e[0].elapsed_time(e[1]) for e in events) / ITERS,
           sum(e[1].elapsed_time(e[2]) for e in events) / ITERS)
    return dev, (host[0] / ITERS * 1e3, host[1] / ITERS * 1e3)


def main():
    if not torch.cuda.is_available():
        sys.exit("ln_microbench needs a GPU")
    s = torch.empty(0, dtype=DTYPE).element_size()
    print(f"dtype {DTYPE}, {ITERS} timed iterations after {WARMUP} warm-up")
    print(f"{'shape':>12} {'p':>4} {'path':>10} {'pass':>4} {'MB':>8} "
          f"{'ms':>8} {'host ms':>8} {'GB/s':>8}  bound")
    for (M, H), p in ((sh, p) for sh in SHAPES for p in PS):
        mod = FusedDropoutAddLayerNorm(H, p=p).cuda().train()
        x = torch.randn(M, H, device="cuda", dtype=DTYPE, requires_grad=True)
        res = torch.randn(M, H, device="cuda", dtype=DTYPE,
                          requires_grad=True)
        dy = torch.randn(M, H, device="cuda", dtype=DTYPE)
        # the composite in the same dtype: parameters cast once, outside the
        # timed region
        w = mod.weight.detach().to(DTYPE).requires_grad_(True)
        b = mod.bias.detach().to(DTYPE).requires_grad_(True)

        def composite(x_, r_):
            return F.layer_norm(r_ + F.dropout(x_, p, True), (H,), w, b,
                                mod.eps)

        nbytes = pass_bytes(M, H, p, s)
        for label, fn in (("fused", mod), ("composite", composite)):
            if label not in PATHS:
                continue
            dev, host = time_passes(fn, x, res, dy)
            for name, nb, t, h in zip(("fwd", "bwd"), nbytes, dev, host):
                # the host took at least 0.8 of the interval to issue the pass
                bound = "host" if h >= 0.8 * t else "device"
                print(f"{M:>6}x{H:<5} {p:>4} {label:>10} {name:>4} "
                      f"{nb / 1e6:8.2f} {t:8.4f} {h:8.4f} "
                      f"{nb / t / 1e6:8.1f}  {bound}")


if __name__ == "__main__":
    main()
