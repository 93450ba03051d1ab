"""Microbench of the masked-row gather (horovod_amd.ops.gather_labelled_rows,
csrc/rows_kernels.hip) at BERT-large pretraining shapes: ids [B, S], H = 1024,
bf16, int(0.15 S) labelled positions per sequence, capacity = B *
max_predictions.

Part one issues each kernel ROWS_ITERS times between device events: the index
build in both variants (one launch with recounting blocks, two launches with
per-chunk counts), the gather, the scatter, and next to them the composite
(nonzero + index_select, which reads the count on the host, and its autograd
backward).  Such a loop measures launch-to-launch time; kernel times come from
a kernel trace of this script (ROWS_PARTS=kernels).  Bytes the kernels have to
move, M = B * S rows, n labelled, 2-byte rows:
  rows_index_k    reads 8 M, writes 4 M + 12 capacity
  rows_gather_k   reads 2 H n, writes 2 H capacity
  rows_scatter_k  reads 4 M + 2 H n, writes 2 H M

Part two is the MLM head, forward + backward between device events: Linear +
GELU + LayerNorm, the tied vocabulary GEMM and softmax_cross_entropy(...,
bias=), on the gathered rows against all M rows.  The two alternate in one
process, ROWS_REPEATS rounds of ROWS_ITERS iterations, and every round's mean
is printed with the host's time to issue an iteration.
Needs a GPU: a measurement without one would say nothing.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from horovod_amd import _core  # noqa: E402
from horovod_amd.ops import (gather_labelled_rows,  # noqa: E402
                             softmax_cross_entropy)

# (B, S, max_predictions per sequence)
SHAPES = [(64, 128, 20), (16, 512, 76)]
if os.environ.get("ROWS_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["ROWS_SHAPES"].split(",")]
PARTS = os.environ.get("ROWS_PARTS", "kernels,head").split(",")
H, V = 1024, 30522
ITERS = int(os.environ.get("ROWS_ITERS", "50"))
REPEATS = int(os.environ.get("ROWS_REPEATS", "3"))
WARMUP = 10


def make_labels(B, S):
    g = torch.Generator().manual_seed(B * S)
    labels = torch.full((B, S), -100)
    for b in range(B):
        cols = torch.randperm(S, generator=g)[:int(0.15 * S)]
        labels[b, cols] = torch.randint(0, V, (cols.numel(),), generator=g)
    return labels.cuda()


def time_loop(fn, iters):
    """Mean us per call of `iters` calls issued back to back."""
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def kernels(B, S, cap):
    M = B * S
    labels = make_labels(B, S).view(-1)
    x = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
    idx, rank, _, count = _core.masked_rows_index(labels, cap)
    n = int(count)
    d_rows = torch.randn(cap, H, device="cuda", dtype=torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    sel = xg.index_select(0, (labels != -100).nonzero().squeeze(1))
    d_sel = torch.randn_like(sel)
    calls = {
        "index, 1 launch": lambda: _core.masked_rows_index(labels, cap, -100, 1),
        "index, 2 launches": lambda: _core.masked_rows_index(labels, cap, -100,
                                                             2),
        "gather": lambda: _core.masked_rows_gather(x, idx, count),
        "scatter": lambda: _core.masked_rows_scatter(d_rows, rank),
        "composite fwd": lambda: x.index_select(
            0, (labels != -100).nonzero().squeeze(1)),
        "composite bwd": lambda: torch.autograd.grad(sel, xg, d_sel,
                                                     retain_graph=True),
    }
    for name, fn in calls.items():
        time_loop(fn, WARMUP)
        rounds = [time_loop(fn, ITERS) for _ in range(REPEATS)]
        print(f"{B:>4}x{S:<4} {name:>18} us/call: " +
              " ".join(f"{r:8.2f}" for r in rounds))
    nbytes = {"rows_index_k": 12 * M + 12 * cap,
              "rows_gather_k": 2 * H * (n + cap),
              "rows_scatter_k": 4 * M + 2 * H * (n + M)}
    for name, nb in nbytes.items():
        print(f"{B:>4}x{S:<4} {name}: {nb / 1e6:.2f} MB, "
              f"{nb / 8e12 * 1e6:.2f} us at 8 TB/s (n = {n}, capacity {cap})")


def head(B, S, cap):
    torch.manual_seed(0)
    transform = nn.Sequential(nn.Linear(H, H), nn.GELU(),
                              nn.LayerNorm(H)).cuda()
    tok = nn.Parameter(torch.randn(V, H, device="cuda") * 0.02)
    bias = nn.Parameter(torch.zeros(V, device="cuda"))
    h = torch.randn(B, S, H, device="cuda",
                    dtype=torch.bfloat16).requires_grad_(True)
    labels = make_labels(B, S)
    params = [h, tok, bias, *transform.parameters()]

    def gathered():
        rows, row_labels = gather_labelled_rows(h, labels, cap)
        return softmax_cross_entropy(transform(rows) @ tok.t(), row_labels,
                                     ignore_index=-100, bias=bias)

    def full():
        return softmax_cross_entropy(
            transform(h).flatten(0, 1) @ tok.t(), labels.flatten(),
            ignore_index=-100, bias=bias)

    def time_round(fn, iters):
        events, host = [], 0.0
        for _ in range(iters):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            t0 = time.perf_counter()
            fn().backward()
            host += time.perf_counter() - t0
            e[1].record()
            for p in params:
                p.grad = None
            events.append(e)
        torch.cuda.synchronize()
        dev = sum(a.elapsed_time(b) for a, b in events) / iters
        return dev, host / iters * 1e3

    fns = {"gathered": gathered, "full": full}
    with torch.autocast("cuda", torch.bfloat16):
        losses = {n: float(fn().detach()) for n, fn in fns.items()}
        print(f"{B:>4}x{S:<4} loss gathered {losses['gathered']:.6f} "
              f"full {losses['full']:.6f}")
        for fn in fns.values():
            time_round(fn, WARMUP)
        for r in range(REPEATS):
            for n, fn in fns.items():
                dev, host = time_round(fn, ITERS)
                bound = "host" if host >= 0.8 * dev else "device"
                print(f"{B:>4}x{S:<4} head {n:>9} {r:>2} {dev:8.4f} ms "
                      f"(host {host:7.4f})  {bound}")


def main():
    if not torch.cuda.is_available():
        sys.exit("rows_microbench needs a GPU")
    print(f"H {H}, V {V}, bf16; {REPEATS} rounds of {ITERS} iterations after "
          f"{WARMUP} warm-up")
    for B, S, per_seq in SHAPES:
        if "kernels" in PARTS:
            kernels(B, S, B * per_seq)
        if "head" in PARTS:
            head(B, S, B * per_seq)


if __name__ == "__main__":
    main()
