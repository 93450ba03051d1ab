"""Microbench: horovod_amd.ops.self_attention against the stock attention
core of FusedLNEncoderLayer._attention (head split into strided views,
F.scaled_dot_product_attention, head merge by transpose + reshape), both from
the packed in_proj output [B, S, 3E] to the out_proj input [B, S, E], forward
+ backward between device events, bf16, training, with a key padding mask.

The two paths alternate inside every iteration of one process; the whole
window is repeated ATTN_RUNS times and the table gives the mean over the runs
of the per-iteration time with the lowest and the highest run.  "host ms" is
the host's time to issue one forward + backward: where it reaches 0.8 of the
event time the row is marked "host", the device waited and the time is the
host's.  TFLOP/s is the arithmetic the algorithm needs (two S x S x 64
products forward, five backward, 2 * B * heads * S^2 * 64 flop each) over the
event time: an end-to-end rate of the call, not a kernel's share of peak (the
fused backward computes seven products, see docs/benchmarks.md).  Kernel
times come from a kernel trace of this script, one configuration per process
(ATTN_SHAPES, ATTN_PATHS below).
Needs a GPU: a measurement without one would say nothing.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from horovod_amd.ops import self_attention  # noqa: E402

# B x heads x S: BERT-large at the benchmark's batch, S = 128 and 512
SHAPES = [(8, 16, 128), (8, 16, 512)]
PATHS = ["fused", "stock"]
# one configuration per process for a kernel trace, e.g.
# ATTN_SHAPES=8x16x128 ATTN_PATHS=fused
if os.environ.get("ATTN_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["ATTN_SHAPES"].split(",")]
if os.environ.get("ATTN_PATHS"):
    PATHS = os.environ["ATTN_PATHS"].split(",")
DTYPE = torch.bfloat16
P = float(os.environ.get("ATTN_P", "0.1"))
ITERS = int(os.environ.get("ATTN_ITERS", "200"))
RUNS = int(os.environ.get("ATTN_RUNS", "5"))
WARMUP = 20


def stock(qkv, heads, pad, p):
    b, s, e3 = qkv.shape
    q, k, v = (t.view(b, s, heads, 64).transpose(1, 2)
               for t in qkv.chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(
        q, k, v, attn_mask=~pad[:, None, None, :], dropout_p=p)
    return o.transpose(1, 2).reshape(b, s, e3 // 3)


def window(fns, qkv, dout, iters):
    """-> per path: (device ms, host ms) per forward + backward"""
    events, host = [[] for _ in fns], [0.0 for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            t0 = time.perf_counter()
            fn(qkv).backward(dout)
            host[k] += time.perf_counter() - t0
            e1.record()
            qkv.grad = None
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    return [(sum(a.elapsed_time(b) for a, b in ev) / iters, h / iters * 1e3)
            for ev, h in zip(events, host)]


def main():
    if not torch.cuda.is_available():
        sys.exit("attn_microbench needs a GPU")
    print(f"dtype {DTYPE}, p {P}, {RUNS} runs of {ITERS} iterations after "
          f"{WARMUP} warm-up, paths alternating")
    print(f"{'B x heads x S':>14} {'path':>6} {'ms':>8} {'min':>8} {'max':>8} "
          f"{'host ms':>8} {'TFLOP/s':>8}  bound")
    for B, H, S in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3 * 64 * H, device="cuda", dtype=DTYPE,
                          generator=g).requires_grad_(True)
        dout = torch.randn(B, S, 64 * H, device="cuda", dtype=DTYPE,
                           generator=g)
        # sequence b keeps S - b * S / 16 keys
        lengths = torch.tensor([S - b * S // 16 for b in range(B)])
        pad = (torch.arange(S)[None, :] >= lengths[:, None]).cuda()
        paths = {"fused": lambda x: self_attention(x, H, pad, P, True),
                 "stock": lambda x: stock(x, H, pad, P)}
        names = [n for n in paths if n in PATHS]
        fns = [paths[n] for n in names]
        window(fns, qkv, dout, WARMUP)
        runs = [window(fns, qkv, dout, ITERS) for _ in range(RUNS)]
        flop = 7 * 2.0 * B * H * S * S * 64
        for k, name in enumerate(names):
            ms = [r[k][0] for r in runs]
            mean, h = sum(ms) / RUNS, sum(r[k][1] for r in runs) / RUNS
            bound = "host" if h >= 0.8 * mean else "device"
            print(f"{B:>4}x{H}x{S:<6} {name:>6} {mean:8.4f} {min(ms):8.4f} "
                  f"{max(ms):8.4f} {h:8.4f} {flop / mean / 1e9:8.2f}  {bound}")


if __name__ == "__main__":
    main()
