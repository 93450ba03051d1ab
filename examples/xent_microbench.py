"""Microbench: horovod_amd.ops.softmax_cross_entropy against F.cross_entropy,
both under bf16 autocast on bf16 logits [M, 30522] with every label valid (no
row is ignored, so the fused backward reads every row), forward + backward
timed as one interval between device events.  The two paths alternate in one
process; after warm-up each of XENT_REPEATS windows runs as many rounds as
make it at least XENT_WINDOW seconds long, and the spread over the windows is
printed next to their mean.

It also prints the bytes each path has to move, computed from the shapes
(E = M * V elements):
  fused  forward reads the bf16 logits (2 E); backward reads them and writes
         the bf16 gradient (4 E); plus M labels and a few floats per row
  stock  autocast casts up (reads 2 E, writes 4 E), log_softmax reads and
         writes fp32 (8 E), nll_loss backward writes an fp32 gradient (4 E),
         log_softmax backward reads two fp32 tensors and writes one (12 E),
         the cast's backward reads fp32 and writes bf16 (6 E): 36 E
and the peak of torch's allocator over one forward + backward of each path,
above what the logits and labels hold.  bytes / time is an end-to-end rate of
the call (launches and allocator included), not a kernel's share of peak;
kernel times come from a kernel trace of this script, one path per process
(XENT_SHAPES=8192x30522 XENT_PATHS=fused).

--bias times the loss of logits + bias instead, bias an fp32 [V] parameter as
BERT's mlm_bias is, both paths through softmax_cross_entropy:
  added   softmax_cross_entropy(x + b, y): ATen adds (reads 2 E, writes 4 E),
          the kernels read fp32 (4 E forward, 4 E + 4 E backward), autograd
          casts the gradient down (6 E) and sums it over rows (4 E): 28 E
  folded  softmax_cross_entropy(x, y, bias=b): 6 E as above, plus the partial
          rows of the bias gradient, written once and read once
Every label is valid here too, so the folded forward skips no row.
Needs a GPU: a measurement without one would say nothing.
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from horovod_amd import _core  # noqa: E402
from horovod_amd.ops import softmax_cross_entropy  # noqa: E402

BIAS = "--bias" in sys.argv[1:]
SHAPES = [(1024, 30522), (8192, 30522)]
PATHS = ["added", "folded"] if BIAS else ["fused", "stock"]
if os.environ.get("XENT_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["XENT_SHAPES"].split(",")]
if os.environ.get("XENT_PATHS"):
    PATHS = os.environ["XENT_PATHS"].split(",")
WINDOW = float(os.environ.get("XENT_WINDOW", "0.5"))
REPEATS = int(os.environ.get("XENT_REPEATS", "3"))
WARMUP = 5
FNS = {"fused": lambda x, y, b: softmax_cross_entropy(x, y),
       "stock": lambda x, y, b: F.cross_entropy(x, y),
       "added": lambda x, y, b: softmax_cross_entropy(x + b, y),
       "folded": lambda x, y, b: softmax_cross_entropy(x, y, bias=b)}


def path_bytes(M, V):
    E = M * V
    # partial rows of the bias gradient: phase classes x row chunks
    rows = (16 // math.gcd(16, V * 2 % 16) *
            _core.fused_xent_bias_row_chunks(M, V, torch.bfloat16))
    return {"fused": 6 * E + 8 * M + 12 * M, "stock": 36 * E + 8 * M,
            "added": 28 * E + 8 * M + 12 * M,
            "folded": 6 * E + 8 * M + 12 * M + 8 * rows * V}


def step(fn, x, y, b):
    with torch.autocast("cuda", torch.bfloat16):
        loss = fn(x, y, b)
    loss.backward()
    x.grad = b.grad = None


def window(names, x, y, b, rounds):
    """ms per forward + backward of each path over `rounds` alternating
    rounds, from device events around every call"""
    marks = []
    for _ in range(rounds):
        for n in names:
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            step(FNS[n], x, y, b)
            e1.record()
            marks.append((n, e0, e1))
    torch.cuda.synchronize()
    return {n: sum(a.elapsed_time(b) for m, a, b in marks if m == n) / rounds
            for n in names}


def peak_bytes(fn, x, y, b):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(fn, x, y, b)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    if not torch.cuda.is_available():
        sys.exit("xent_microbench needs a GPU")
    names = [n for n in FNS if n in PATHS]
    print(f"bf16 logits{' + fp32 bias' if BIAS else ''} under bf16 autocast, "
          f"forward + backward; {REPEATS} "
          f"windows of at least {WINDOW} s after {WARMUP} warm-up rounds")
    print(f"{'shape':>12} {'path':>6} {'MB moved':>9} {'ms':>8} {'min':>8} "
          f"{'max':>8} {'GB/s':>8} {'peak MB':>9}")
    for M, V in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + V)
        x = torch.randn(M, V, device="cuda", generator=g).bfloat16()
        x.requires_grad_(True)
        y = torch.randint(0, V, (M,), device="cuda", generator=g)
        b = torch.randn(V, device="cuda", generator=g).requires_grad_(True)
        for _ in range(WARMUP):
            window(names, x, y, b, 1)
        per_round = sum(window(names, x, y, b, 5).values()) / 1e3
        rounds = max(10, int(WINDOW / per_round) + 1)
        runs = [window(names, x, y, b, rounds) for _ in range(REPEATS)]
        nbytes = path_bytes(M, V)
        for n in names:
            ts = [r[n] for r in runs]
            t = sum(ts) / len(ts)
            print(f"{M:>6}x{V:<5} {n:>6} {nbytes[n] / 1e6:9.1f} {t:8.4f} "
                  f"{min(ts):8.4f} {max(ts):8.4f} {nbytes[n] / t / 1e6:8.1f} "
                  f"{peak_bytes(FNS[n], x, y, b) / 1e6:9.1f}")


if __name__ == "__main__":
    main()
