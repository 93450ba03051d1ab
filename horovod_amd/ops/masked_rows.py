"""Gather of the labelled rows, backed by the CDNA4 kernels in
csrc/rows_kernels.hip: of x [..., H] and labels [...], the rows whose label is
not ignore_index, in rising position, as rows [capacity, H] with their labels
[capacity].  It is what a BERT MLM head runs on instead of all B * S rows.

Three kernels and no host read: the index build (positions of the labelled
rows, their inverse, the compacted labels and the count), the gather, and for
the backward one pass that writes every element of the gradient of x once,
the rows that were not gathered as zeros.  No memset and no atomics, so
identical inputs give identical bits.

Rows [count, capacity) are zeros and carry the label ignore_index, so a loss
with that ignore_index skips them.  When more than capacity rows are labelled
every element of rows is NaN (row_labels then holds the first capacity
labels): the loss becomes NaN and a loss scaler skips the step, with no host
read to find out.

capacity=None is the convenient form, and it synchronises: the count is read
on the host once and rounded up to a multiple of 8, at least 8.

Input the kernels do not take (CPU tensors, rows that are not fp32, fp16 or
bf16, H * itemsize not a multiple of 16, non-contiguous or misaligned x or
labels, labels that are not int64) goes through a composite on torch indexing
with the same results.
"""
import torch

from horovod_amd import _core
from horovod_amd.ops.fused_ln import _DTYPES, _act_ok

# labels per block of the index build (kRowsChunk, csrc/kernels.h)
INDEX_CHUNK = _core.masked_rows_chunk()
_MAX_M = 2 ** 31 - 1
_MAX_ROW_BYTES = 1 << 24


def _ceil8(n):
    return max(8, (n + 7) // 8 * 8)


def _composite(x, labels, capacity, ignore_index):
    pos = (labels != ignore_index).nonzero().squeeze(1)
    n = pos.numel()
    if capacity is None:
        capacity = _ceil8(n)
    pos = pos[:capacity]
    row_labels = labels.new_full((capacity,), ignore_index)
    row_labels[:pos.numel()] = labels[pos]
    rows = x.index_select(0, pos)
    if n > capacity:
        return rows + float("nan"), row_labels
    return torch.cat([rows, x.new_zeros(capacity - n, x.shape[1])]), row_labels


def _eligible(x, labels, capacity):
    """True when the native kernels take this call."""
    row_bytes = x.shape[1] * x.element_size()
    return (x.dtype in _DTYPES and _act_ok(x) and
            labels.dtype == torch.int64 and _act_ok(labels) and
            labels.device == x.device and 1 <= x.shape[0] <= _MAX_M and
            16 <= row_bytes <= _MAX_ROW_BYTES and row_bytes % 16 == 0 and
            (capacity is None or capacity <= _MAX_M))


class _GatherLabelledRowsFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, labels, capacity, ignore_index):
        if capacity is None:
            # room for every row, then cut to the count read on the host
            idx, rank, row_labels, count = _core.masked_rows_index(
                labels, _ceil8(labels.numel()), ignore_index)
            capacity = _ceil8(int(count.item()))
            idx, row_labels = idx[:capacity], row_labels[:capacity]
        else:
            idx, rank, row_labels, count = _core.masked_rows_index(
                labels, capacity, ignore_index)
        rows = _core.masked_rows_gather(x, idx, count)
        ctx.save_for_backward(rank)
        ctx.mark_non_differentiable(row_labels)
        return rows, row_labels

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_rows, _):
        rank, = ctx.saved_tensors
        # the forward checked its inputs; the incoming gradient can still be
        # strided, or a contiguous view at an offset the 16-B loads cannot take
        d_rows = d_rows.contiguous()
        if d_rows.data_ptr() % 16 != 0:
            d_rows = d_rows.clone()
        return _core.masked_rows_scatter(d_rows, rank), None, None, None


def gather_labelled_rows(x, labels, capacity=None, ignore_index=-100):
    """-> (rows [capacity, H], row_labels [capacity]) of x [..., H] and integer
    labels [...] of the same leading shape: the rows whose label is not
    ignore_index, in rising position; zeros and ignore_index from their count
    on; all of rows NaN when the count exceeds capacity.  capacity=None reads
    the count on the host and takes it rounded up to a multiple of 8, at least
    8."""
    if x.dim() < 1 or tuple(labels.shape) != tuple(x.shape[:-1]):
        raise ValueError(
            f"labels have to have the leading shape of x, but got "
            f"{tuple(labels.shape)} for x {tuple(x.shape)}")
    if labels.dtype.is_floating_point or labels.dtype.is_complex or \
            labels.dtype == torch.bool:
        raise ValueError(f"labels have to be integers, got {labels.dtype}")
    if capacity is not None:
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity has to be at least 1, got {capacity}")
    x2, labels1 = x.reshape(-1, x.shape[-1]), labels.reshape(-1)
    if _eligible(x2, labels1, capacity):
        return _GatherLabelledRowsFn.apply(x2, labels1, capacity,
                                           int(ignore_index))
    return _composite(x2, labels1, capacity, ignore_index)
