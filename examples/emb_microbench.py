"""Microbench of the BERT input block: horovod_amd.ops.embedding_layer_norm on
the fused kernels against the composite the model runs without fused_emb
(three nn.Embedding lookups, two adds, LayerNorm, dropout), forward + backward
under bf16 autocast with fp32 tables, timed between device events.

The two paths alternate in one process, EMB_REPEATS rounds of EMB_ITERS
iterations each, and the mean of every round is printed with the host's time
to issue an iteration, so the spread between rounds is visible and a row in
which the device waited for the host is marked.  Kernel times come from a
kernel trace of this script with one path per process (EMB_PATHS=fused or
EMB_PATHS=composite).  Bytes the fused kernels have to move, M = B * S rows,
fp32 tables, 2-byte activations:
  emb_ln_fwd_k   reads M token rows (4 H), writes y (2 H): 6 M H
  emb_ln_bwd_k   reads dy (2 H) and M token rows (4 H), writes dz (4 H):
                 10 M H, plus the partial rows
  emb_scatter_k  reads dz (4 M H), writes the table's gradient (4 V H)
Needs a GPU: a measurement without one would say nothing.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from horovod_amd.ops import embedding_layer_norm  # noqa: E402

SHAPES = [(64, 128), (16, 512)]
PATHS = ["fused", "composite"]
if os.environ.get("EMB_SHAPES"):
    SHAPES = [tuple(int(v) for v in sh.split("x"))
              for sh in os.environ["EMB_SHAPES"].split(",")]
if os.environ.get("EMB_PATHS"):
    PATHS = os.environ["EMB_PATHS"].split(",")
H, V, P, DROP = 1024, 30522, 512, 0.1
ITERS = int(os.environ.get("EMB_ITERS", "50"))
REPEATS = int(os.environ.get("EMB_REPEATS", "3"))
WARMUP = 10


def kernel_bytes(M):
    return {"emb_ln_fwd_k": 6 * M * H, "emb_ln_bwd_k": 10 * M * H,
            "emb_scatter_k": 4 * M * H + 4 * V * H}


def time_round(fn, params, dy, iters):
    """Mean ms of forward + backward between device events, and on the host
    clock around issuing them (no synchronise inside the window)."""
    events, host = [], 0.0
    for _ in range(iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        t0 = time.perf_counter()
        fn().backward(dy)
        host += time.perf_counter() - t0
        e[1].record()
        for p in params:
            p.grad = None
        events.append(e)
    torch.cuda.synchronize()
    dev = sum(a.elapsed_time(b) for a, b in events) / iters
    return dev, host / iters * 1e3


def main():
    if not torch.cuda.is_available():
        sys.exit("emb_microbench needs a GPU")
    print(f"H {H}, V {V}, bf16 autocast, p {DROP}; {REPEATS} rounds of "
          f"{ITERS} iterations after {WARMUP} warm-up")
    print(f"{'ids':>9} {'path':>10} {'round':>5} {'ms':>8} {'host ms':>8}  "
          "bound")
    for B, S in SHAPES:
        torch.manual_seed(0)
        tok, pos, typ = (nn.Embedding(n, H).cuda() for n in (V, P, 2))
        norm, drop = nn.LayerNorm(H).cuda(), nn.Dropout(DROP)
        ids = torch.randint(0, V, (B, S), device="cuda")
        types = torch.randint(0, 2, (B, S), device="cuda")
        arange = torch.arange(S, device="cuda").unsqueeze(0)
        params = [tok.weight, pos.weight, typ.weight, norm.weight, norm.bias]

        def fused():
            return embedding_layer_norm(ids, types, *params, p=DROP,
                                        eps=norm.eps)

        def composite():
            return drop(norm(tok(ids) + pos(arange) + typ(types)))

        fns = {"fused": fused, "composite": composite}
        with torch.autocast("cuda", torch.bfloat16):
            dys = {n: torch.randn_like(fns[n]()) for n in PATHS}
            for n in PATHS:
                time_round(fns[n], params, dys[n], WARMUP)
            for r in range(REPEATS):
                for n in PATHS:
                    dev, host = time_round(fns[n], params, dys[n], ITERS)
                    bound = "host" if host >= 0.8 * dev else "device"
                    print(f"{B:>4}x{S:<4} {n:>10} {r:>5} {dev:8.4f} "
                          f"{host:8.4f}  {bound}")
        for name, nb in kernel_bytes(B * S).items():
            print(f"{B:>4}x{S:<4} {name}: {nb / 1e6:.1f} MB, "
                  f"{nb / 8e12 * 1e6:.1f} us at 8 TB/s")


if __name__ == "__main__":
    main()
