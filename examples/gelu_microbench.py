"""Per-pass microbench: bias_gelu_dropout against the composite
F.dropout(F.gelu(u + bias)) in the same dtype (bf16, training), forward and
backward timed apart with device events, the two paths alternating in one
process.

For each pass it prints the bytes the fused pass has to move, computed from
the shapes, the time between the device events, the host's time to issue the
pass, and bytes over the event time.  That quotient is an end-to-end rate of
the pass (launches and allocator included, not a kernel's share of peak), and
only where the row is marked "device": in a row marked "host" the device
waited for the host, and the time is the host's.  Kernel times come from a
kernel trace of this script, one configuration per process (GELU_SHAPES,
GELU_PS, GELU_PATHS below).  With E = M * N elements of s bytes:
  forward   reads u, writes out: 2 * E * s, plus N bias values
  backward  reads dy and u, writes du: 3 * E * s, plus the partial rows of
            the bias gradient, written and read once: 2 * chunks * N * 4
The composite moves more (docs/benchmarks.md counts it); its rows carry the
same MB so that the two GB/s columns compare times, not traffic.
Needs a GPU: a measurement without one would say nothing.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from horovod_amd import _core  # noqa: E402
from horovod_amd.ops import bias_gelu_dropout  # noqa: E402

SHAPES = [(1024, 4096), (8192, 3072), (16384, 4096)]
PS = [0.1, 0.0]
PATHS = ["fused", "composite"]
# one configuration per process for a kernel trace, e.g.
# GELU_SHAPES=8192x3072 GELU_PS=0.1 GELU_PATHS=fused
if os.environ.get("GELU_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["GELU_SHAPES"].split(",")]
if os.environ.get("GELU_PS"):
    PS = [float(v) for v in os.environ["GELU_PS"].split(",")]
if os.environ.get("GELU_PATHS"):
    PATHS = os.environ["GELU_PATHS"].split(",")
DTYPE = torch.bfloat16
ITERS = int(os.environ.get("GELU_ITERS", "50"))
WARMUP = 10


def pass_bytes(M, N, s):
    chunks = _core.fused_bias_gelu_row_chunks(M, N)
    return (2 * M * N * s + N * 4,
            3 * M * N * s + N * 4 + (2 * chunks * N * 4 if chunks > 1 else 0))


def time_round(fns, u, dy, dev, host):
    """One forward and backward of every path in turn, device events and the
    host clock around issuing each pass (no synchronise inside)."""
    events = []
    for k, fn in enumerate(fns):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        t0 = time.perf_counter()
        y = fn(u)
        t1 = time.perf_counter()
        e[1].record()
        y.backward(dy)
        t2 = time.perf_counter()
        e[2].record()
        u.grad = None
        events.append(e)
        if host is not None:
            host[k][0] += t1 - t0
            host[k][1] += t2 - t1
    if dev is not None:
        dev.append(events)


def main():
    if not torch.cuda.is_available():
        sys.exit("gelu_microbench needs a GPU")
    s = torch.empty(0, dtype=DTYPE).element_size()
    print(f"dtype {DTYPE}, {ITERS} timed iterations after {WARMUP} warm-up")
    print(f"{'shape':>12} {'p':>4} {'path':>10} {'pass':>4} {'MB':>8} "
          f"{'ms':>8} {'host ms':>8} {'GB/s':>8}  bound")
    for (M, N), p in ((sh, p) for sh in SHAPES for p in PS):
        u = torch.randn(M, N, device="cuda", dtype=DTYPE, requires_grad=True)
        dy = torch.randn(M, N, device="cuda", dtype=DTYPE)
        bias = torch.randn(N, device="cuda", requires_grad=True)
        # the composite in the same dtype: bias cast once, outside the timing
        bias_t = bias.detach().to(DTYPE).requires_grad_(True)
        paths = {
            "fused": lambda x: bias_gelu_dropout(x, bias, p, True),
            "composite": lambda x: F.dropout(F.gelu(x + bias_t), p, True),
        }
        names = [n for n in paths if n in PATHS]
        fns = [paths[n] for n in names]
        for _ in range(WARMUP):
            time_round(fns, u, dy, None, None)
        # One synchronise for the whole window.  The events bracket device
        # work only while the host issues a pass faster than the device runs
        # it; rows where it does not are marked host-bound below.
        torch.cuda.synchronize()
        dev, host = [], [[0.0, 0.0] for _ in fns]
        for _ in range(ITERS):
            time_round(fns, u, dy, dev, host)
        torch.cuda.synchronize()
        nbytes = pass_bytes(M, N, s)
        for k, label in enumerate(names):
            for j, name in enumerate(("fwd", "bwd")):
                t = sum(r[k][j].elapsed_time(r[k][j + 1]) for r in dev) / ITERS
                h = host[k][j] / ITERS * 1e3
                # the host took at least 0.8 of the interval to issue the pass
                bound = "host" if h >= 0.8 * t else "device"
                print(f"{M:>6}x{N:<5} {p:>4} {label:>10} {name:>4} "
                      f"{nbytes[j] / 1e6:8.2f} {t:8.4f} {h:8.4f} "
                      f"{nbytes[j] / t / 1e6:8.1f}  {bound}")


if __name__ == "__main__":
    main()
