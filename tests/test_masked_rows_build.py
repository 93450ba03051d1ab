"""The masked-row gather without a GPU: the binding surface, the composite of
gather_labelled_rows on CPU tensors against torch indexing (reference() below,
which tests/test_gpu_masked_rows.py shares), its ValueErrors, and the BERT MLM
head on the gathered rows against the head on all rows.

The BERT comparison is in fp64 on the CPU in eval(): both paths then differ
only in the order of their sums, around 1e-15 relative, while a dropped or
misplaced row changes the loss in its first digits; the bound of 1e-10 sits
six orders away from both.
"""
import pytest
import torch
import torch.nn.functional as F

from horovod_amd import _core
from horovod_amd.models.bert import (BertConfig, BertForPretraining,
                                     BertPretrainingLoss)
from horovod_amd.ops import gather_labelled_rows

CAPACITIES = ["exact", "plus3", "minus1", None]


def reference(x, labels, capacity, ignore_index=-100):
    """-> pos (the labelled positions), rank, row_labels, rows, capacity, from
    torch indexing on CPU copies.  capacity: an int, None, or one of
    CAPACITIES relative to the count."""
    x, labels = x.cpu().reshape(-1, x.shape[-1]), labels.cpu().reshape(-1)
    pos = (labels != ignore_index).nonzero().squeeze(1)
    n = pos.numel()
    if capacity is None:
        capacity = max(8, (n + 7) // 8 * 8)
    elif isinstance(capacity, str):
        capacity = max(1, n + {"exact": 0, "plus3": 3,
                               "minus1": -1 if n >= 2 else 0}[capacity])
    rank = torch.full((labels.numel(),), -1, dtype=torch.int32)
    rank[pos] = torch.arange(n, dtype=torch.int32)
    kept = pos[:capacity]
    row_labels = torch.full((capacity,), ignore_index, dtype=labels.dtype)
    row_labels[:kept.numel()] = labels[kept]
    rows = torch.zeros(capacity, x.shape[1], dtype=x.dtype)
    rows[:kept.numel()] = x[kept]
    if n > capacity:
        rows.fill_(float("nan"))
    return pos, rank, row_labels, rows, capacity


def reference_dx(d_rows, pos, M):
    kept = pos[:d_rows.shape[0]]
    zeros = torch.zeros(M, d_rows.shape[1], dtype=d_rows.dtype)
    return zeros.index_copy(0, kept, d_rows.cpu()[:kept.numel()])


def same(a, b):
    """torch.equal, with NaN equal to NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(), b.nan_to_num())


def test_binding_surface_and_cpu_tensors():
    for name in ("masked_rows_index", "masked_rows_gather",
                 "masked_rows_scatter"):
        assert hasattr(_core, name)
    labels, ints = torch.zeros(4, dtype=torch.int64), torch.zeros(4).int()
    with pytest.raises(RuntimeError, match="GPU"):
        _core.masked_rows_index(labels, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.masked_rows_gather(torch.zeros(4, 8), ints, ints[:1])
    with pytest.raises(RuntimeError, match="GPU"):
        _core.masked_rows_scatter(torch.zeros(4, 8), ints)


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_composite_on_cpu(capacity):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 7, 6, generator=g, dtype=torch.float64)
    labels = torch.full((3, 7), -100)
    labels[0, 0], labels[1, 3], labels[2, 5], labels[2, 6] = 5, 0, 9, 2
    pos, _, r_labels, r_rows, cap = reference(x, labels, capacity)
    xg = x.clone().requires_grad_(True)
    rows, row_labels = gather_labelled_rows(
        xg, labels, None if capacity is None else cap)
    assert same(rows, r_rows) and torch.equal(row_labels, r_labels)
    assert cap == {"exact": 4, "plus3": 7, "minus1": 3, None: 8}[capacity]
    d_rows = torch.randn(cap, 6, generator=g, dtype=torch.float64)
    rows.backward(d_rows)
    assert torch.equal(xg.grad.view(21, 6), reference_dx(d_rows, pos, 21))


def test_value_errors():
    x, labels = torch.zeros(2, 3, 8), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="leading shape"):
        gather_labelled_rows(x, labels[:, :2])
    with pytest.raises(ValueError, match="integers"):
        gather_labelled_rows(x, labels.float())
    with pytest.raises(ValueError, match="capacity"):
        gather_labelled_rows(x, labels, capacity=0)


def _tiny_bert():
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=100, hidden=128, layers=2, heads=2,
                     intermediate=256, max_seq=16)
    model = BertForPretraining(cfg, fused_ln=False, fused_gelu=False,
                               fused_attn=False, fused_emb=False)
    model = model.double().eval()
    with torch.no_grad():
        model.mlm_bias.normal_()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 100, (3, 16), generator=g)
    types = torch.randint(0, 2, (3, 16), generator=g)
    attn = torch.ones(3, 16, dtype=torch.int64)
    attn[1, 11:] = 0
    labels = torch.full((3, 16), -100)
    for b, cols in enumerate(([0, 5, 15], [2], [1, 3, 4, 7, 8, 9, 12, 13])):
        labels[b, cols] = torch.randint(0, 100, (len(cols),), generator=g)
    return model, ids, types, attn, labels, torch.tensor([0, 1, 1])


def test_bert_head_on_gathered_rows_matches_full_head():
    model, ids, types, attn, labels, nsp_labels = _tiny_bert()
    loss_fn = BertPretrainingLoss(fused=False)
    results = []
    for gathered in (False, True):
        model.zero_grad()
        if gathered:
            mlm, nsp, row_labels = model(ids, types, attn, mlm_labels=labels,
                                         max_predictions=8)
            assert mlm.shape == (24, 100) and row_labels.shape == (24,)
            loss = loss_fn(mlm, nsp, row_labels, nsp_labels)
        else:
            mlm, nsp = model(ids, types, attn)
            loss = loss_fn(mlm, nsp, labels, nsp_labels)
        loss.backward()
        results.append((loss.detach(), {n: p.grad.clone() for n, p in
                                        model.named_parameters()}))
    (full, full_grads), (part, part_grads) = results
    assert abs(part - full) <= 1e-10 * abs(full)
    for name, g in full_grads.items():
        err = (part_grads[name] - g).abs().max()
        assert err <= 1e-10 * g.abs().max(), name


def test_bert_without_labels_is_unchanged():
    model, ids, types, attn, _, _ = _tiny_bert()
    with torch.no_grad():
        mlm, nsp = model(ids, types, attn)
        pos = torch.arange(16).unsqueeze(0)
        x = model.tok_emb(ids) + model.pos_emb(pos) + model.type_emb(types)
        h = model.encoder(model.emb_drop(model.emb_norm(x)),
                          src_key_padding_mask=attn == 0)
        want = model.mlm_transform(h) @ model.tok_emb.weight.t() + \
            model.mlm_bias
        assert torch.equal(mlm, want)
        assert torch.equal(nsp, model.nsp(h[:, 0]))


def test_loss_takes_two_dimensional_logits():
    g = torch.Generator().manual_seed(2)
    mlm, nsp = torch.randn(6, 11, generator=g), torch.randn(2, 2, generator=g)
    labels, nsp_labels = torch.tensor([3, -100, 0, 10, -100, 7]), \
        torch.tensor([1, 0])
    loss = BertPretrainingLoss(fused=False)(mlm, nsp, labels, nsp_labels)
    want = F.cross_entropy(mlm, labels, ignore_index=-100) + \
        F.cross_entropy(nsp, nsp_labels)
    assert torch.equal(loss, want)
