"""The masked-row kernels on the GPU against torch indexing on CPU copies
(reference() of tests/test_masked_rows_build.py).  Gather and scatter are
copies, so every comparison is exact.

M comes from the kernels' constants: C = masked_rows.INDEX_CHUNK (kRowsChunk,
the labels of one block of the index build; a wave ranks 128 of them at a
time, a lane two): 1, 63 / 64 / 65 (a wave of lanes), C - 1, C + 1 and 3 C + 5
(four blocks, the last one short, an odd M).  `launches` picks the index
build's variant: 1 (each block recounts the chunks before it), 2 (per-chunk
counts first), 0 (the rule by length).  (H, dtype): (8, fp16) a single vector,
(72, bf16) nine vectors, no multiple of the gather's 64 lanes and no divisor
of the scatter's 256 threads, (1024, bf16) two vectors per lane, (4, fp32).
Patterns: none / all / 15 % at random / first and last only / a gap (with
three chunks or more: chunk 1 without labels; below, the middle third).
Capacity: exactly count, count + 3 (zero rows and ignore_index labels behind),
count - 1 where count >= 2 (overflow: rows all NaN, count the true number),
and None through the public function.  The cases rotate through these by the
rule in _grid(), not the full product.

Every output is allocated by the binding, so each case runs twice, each time
right after a same-sized allocation filled with another byte was freed: an
element that a kernel does not write shows that byte.  The test of the public
function also checks that its output hangs on the new autograd Function.
"""
import pytest
import torch

from tests.test_masked_rows_build import (CAPACITIES, reference, reference_dx,
                                          same)

pytestmark = pytest.mark.gpu

HD = [(8, torch.float16), (72, torch.bfloat16), (1024, torch.bfloat16),
      (4, torch.float32)]
PATTERNS = ["none", "all", "random", "ends", "gap"]


def _ms():
    from horovod_amd.ops.masked_rows import INDEX_CHUNK as C
    return [1, 63, 64, 65, C - 1, C + 1, 3 * C + 5]


def _grid():
    return [(M, HD[(i + k) % 4], pattern, CAPACITIES[(i + 2 * k) % 3],
             (i + k) % 3)
            for i, M in enumerate(_ms()) for k, pattern in enumerate(PATTERNS)]


def _id(case):
    M, (H, dtype), pattern, capacity, launches = case
    return f"M{M}-H{H}-{str(dtype)[6:]}-{pattern}-{capacity}-l{launches}"


def _inputs(M, H, dtype, pattern):
    from horovod_amd.ops.masked_rows import INDEX_CHUNK as C
    g = torch.Generator().manual_seed(M + PATTERNS.index(pattern))
    on = torch.rand(M, generator=g) < 0.15
    if pattern in ("none", "all"):
        on[:] = pattern == "all"
    elif pattern == "ends":
        on[:] = False
        on[0] = on[-1] = True
    elif pattern == "gap":
        lo, hi = (C, 2 * C) if M >= 3 * C else (M // 3, 2 * M // 3)
        on[0], on[-1] = True, M > 1
        on[lo:hi] = False
    labels = torch.randint(0, 30522, (M,), generator=g)
    labels[~on] = -100
    return torch.randn(M, H, generator=g).to(dtype), labels


def _dirty(byte, *nbytes):
    junk = [torch.full((n,), byte, dtype=torch.uint8, device="cuda")
            for n in nbytes]
    del junk


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_core_kernels(case):
    from horovod_amd import _core
    M, (H, dtype), pattern, capacity, launches = case
    x, labels = _inputs(M, H, dtype, pattern)
    pos, r_rank, r_labels, r_rows, cap = reference(x, labels, capacity)
    d_rows = torch.randn(cap, H).to(dtype)
    r_dx = reference_dx(d_rows, pos, M)
    xd, ld, dd = x.cuda(), labels.cuda(), d_rows.cuda()
    for byte in (0x55, 0xAA):
        # idx, rank, row_labels, count, rows, dx
        _dirty(byte, 4 * cap, 4 * M, 8 * cap, 4, xd.element_size() * cap * H,
               xd.element_size() * M * H)
        idx, rank, row_labels, count = _core.masked_rows_index(
            ld, cap, -100, launches)
        rows = _core.masked_rows_gather(xd, idx, count)
        dx = _core.masked_rows_scatter(dd, rank)
        n = pos.numel()
        assert int(count) == n
        assert torch.equal(idx[:n].cpu(), pos[:cap].int())
        assert torch.equal(idx[n:].cpu(), torch.full((max(cap - n, 0),), -1,
                                                     dtype=torch.int32))
        assert torch.equal(rank.cpu(), r_rank)
        assert torch.equal(row_labels.cpu(), r_labels)
        assert same(rows, r_rows)
        assert torch.equal(dx.cpu(), r_dx)
        del idx, rank, row_labels, count, rows, dx


@pytest.mark.parametrize("case", _grid()[2::3], ids=_id)
@pytest.mark.parametrize("capacity", ["plus3", None])
def test_gather_labelled_rows(case, capacity):
    from horovod_amd.ops import gather_labelled_rows
    M, (H, dtype), pattern, _, _ = case
    x, labels = _inputs(M, H, dtype, pattern)
    pos, _, r_labels, r_rows, cap = reference(x, labels, capacity)
    xd = x.cuda().requires_grad_(True)
    rows, row_labels = gather_labelled_rows(
        xd, labels.cuda(), None if capacity is None else cap)
    assert same(rows, r_rows) and torch.equal(row_labels.cpu(), r_labels)
    assert type(rows.grad_fn).__name__ == "_GatherLabelledRowsFnBackward"
    d_rows = torch.randn(cap, H).to(dtype)
    # a strided gradient: the backward has to make it contiguous
    rows.backward(d_rows.cuda().t().contiguous().t())
    assert torch.equal(xd.grad.cpu(), reference_dx(d_rows, pos, M))


def test_two_runs_are_bitwise_equal():
    from horovod_amd.ops import gather_labelled_rows
    M, H = _ms()[-1], 1024
    x, labels = _inputs(M, H, torch.bfloat16, "random")
    labels = labels.view(-1, 1).cuda()
    runs = []
    for _ in range(2):
        xd = x.view(M, 1, H).cuda().requires_grad_(True)
        rows, row_labels = gather_labelled_rows(xd, labels, M // 4)
        rows.backward(torch.ones_like(rows) * 3)
        runs.append((rows.detach().view(torch.int16), row_labels,
                     xd.grad.view(torch.int16)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
