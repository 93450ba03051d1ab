"""Fused softmax cross-entropy with the bias folded in, on the GPU against
fp64: F.cross_entropy(x.double() + b.double(), y, ...) on CPU copies of the
dtype-rounded logits and the fp32 bias, its autograd gradients for a random
incoming gradient, and torch.logsumexp.

|err| <= tol + tol * |ref| (_close), the figures of test_gpu_fused_xent.py:
loss, row loss, lse (rows that are not ignored; the others are not read) and
dbias 2e-4, dx 2e-4 (fp32), 2^-8 (bf16), 2^-10 (fp16).  dbias is an fp32 sum of
fp32 values over at most 129 rows: the same formula evaluated in fp32 on the
CPU and summed in row order reaches 4.4e-3 of the dbias bound at worst over
the whole grid below, far under the quarter that would have widened it.

Grid: V {1, 7, 8, 9, 1031, 2057, 30522} x M {1, 9, 67}.  1, 7: classes of a
head only; 8, 9: one vector and a one-element tail; 1031: odd, eight phase
classes for 2-byte types and four for fp32; 2057: a second column tile of a
few vectors; 30522: the real shape, four classes.  M = 1 leaves classes empty,
9 gives classes of unequal size, 67 is ragged.  With V = 1031 and 2057 also
the smallest M that gives a class two row chunks, the last one short.  dtype,
smoothing, reduction and "every third row ignored" rotate as in
test_gpu_fused_xent.py.  Logits are 4 * randn with row 0 shifted by +50 and
the last row by -50; the bias is 2 * randn with one entry at +30, which a
kernel that drops the bias cannot survive.
"""
import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_fused_ln import _bert_batch, _close, _tiny_bert

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
REDUCTIONS = ["none", "mean", "sum"]
ROWS = [1, 9, 67]
VS = [1, 7, 8, 9, 1031, 2057, 30522]
TOL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
IGNORE = -100
CHUNKED = "two chunks"  # stands for the M that _rows() takes from the core


def _core():
    from horovod_amd import _core
    return _core


def _phases(V, dtype):
    return 16 // math.gcd(16, V * dtype.itemsize % 16)


def _rows(M, V, dtype):
    if M != CHUNKED:
        return M
    chunks = functools.partial(_core().fused_xent_bias_row_chunks, V=V,
                               dtype=dtype)
    M = next(m for m in range(1, 1024) if chunks(m) >= 2)
    assert -(-M // _phases(V, dtype)) % chunks(M) != 0  # a short last chunk
    return M


def _grid():
    cases = []
    for i, (M, V) in enumerate(itertools.product(ROWS, VS)):
        r, c = divmod(i, len(VS))
        n = c + r
        cases.append((M, V, DTYPES[n % 3], 0.1 * (n % 2),
                      REDUCTIONS[(c + 2 * r) % 3], n // 2 % 2 == 1))
    return cases + [(CHUNKED, 1031, torch.bfloat16, 0.1, "mean", True),
                    (CHUNKED, 2057, torch.float32, 0.0, "sum", False),
                    (CHUNKED, 2057, torch.float16, 0.1, "none", True)]


def _id(case):
    M, V, dtype, eps, reduction, ignoring = case
    return (f"{M}x{V}-{str(dtype)[6:]}-eps{eps}-{reduction}-"
            f"{'ignore' if ignoring else 'all'}")


@functools.lru_cache(maxsize=None)
def _case(M, V, dtype, eps, reduction, ignoring, ignore_from=2, ignore_step=3):
    """dtype-rounded CPU inputs and the fp64 reference: (x, b, y, dloss),
    (loss, row loss, lse, dx, dbias)"""
    M = _rows(M, V, dtype)
    g = torch.Generator().manual_seed(7 * M + V)
    x = 4 * torch.randn(M, V, generator=g)
    x[0] += 50
    x[-1] -= 50
    x = x.to(dtype)
    b = 2 * torch.randn(V, generator=g)
    b[V // 2] = 30
    y = torch.randint(0, V, (M,), generator=g)
    if ignoring:
        y[ignore_from::ignore_step] = IGNORE
    dloss = torch.randn(M if reduction == "none" else 1, generator=g)
    xd = x.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    kw = dict(label_smoothing=eps, ignore_index=IGNORE)
    loss = F.cross_entropy(xd + bd, y, reduction=reduction, **kw)
    dx, db = torch.autograd.grad(loss, (xd, bd),
                                 dloss.double().view(loss.shape))
    z = (xd + bd).detach()
    rows = F.cross_entropy(z, y, reduction="none", **kw)
    return (x, b, y, dloss), (loss.detach(), rows, torch.logsumexp(z, 1), dx,
                              db)


def _run_native(x, b, y, dloss, eps, reduction):
    core = _core()
    x, b, y = x.cuda(), b.cuda(), y.cuda()
    loss, rows, lse, count = core.fused_xent_bias_forward(x, b, y, eps, IGNORE,
                                                          reduction)
    dx, db = core.fused_xent_bias_backward(dloss.cuda(), x, b, y, lse, count,
                                           eps, IGNORE, reduction)
    return loss, rows, lse, count, dx, db


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_matches_fp64_reference(case):
    _, V, dtype, eps, reduction, ignoring = case
    (x, b, y, dloss), (r_loss, r_rows, r_lse, r_dx, r_db) = _case(*case)
    loss, rows, lse, count, dx, db = _run_native(x, b, y, dloss, eps,
                                                 reduction)
    assert loss.dtype == lse.dtype == count.dtype == db.dtype == torch.float32
    assert dx.dtype == dtype
    assert float(count) == int((y != IGNORE).sum())
    _close(loss, r_loss, 2e-4, "loss")
    if reduction == "none":
        assert rows is None
    else:
        _close(rows, r_rows, 2e-4, "row loss")
    _close(lse.cpu()[y != IGNORE], r_lse[y != IGNORE], 2e-4, "lse")
    _close(dx, r_dx, TOL[dtype], "dx")
    _close(db, r_db, 2e-4, "dbias")
    assert not bool(dx.cpu()[y == IGNORE].any())


def test_whole_class_ignored():
    """rows 0, 8, 16, ... are all of class 0 of a bf16 row of 1031"""
    case = (67, 1031, torch.bfloat16, 0.1, "mean", True, 0, 8)
    (x, b, y, dloss), (_, _, _, r_dx, r_db) = _case(*case)
    *_, dx, db = _run_native(x, b, y, dloss, 0.1, "mean")
    assert not bool(dx[0::8].any())
    _close(dx, r_dx, TOL[torch.bfloat16], "dx")
    _close(db, r_db, 2e-4, "dbias")


def test_bitwise_reproducible():
    (x, b, y, dloss), _ = _case(67, 30522, torch.bfloat16, 0.1, "mean", True)
    runs = [_run_native(x, b, y, dloss, 0.1, "mean") for _ in range(2)]
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_public_function():
    from horovod_amd.ops import softmax_cross_entropy
    case = (9, 1031, torch.bfloat16, 0.1, "mean", True)
    (x, b, y, dloss), (r_loss, _, _, r_dx, r_db) = _case(*case)
    xg = x.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        loss = softmax_cross_entropy(xg, y.cuda(), 0.1, IGNORE, "mean", bg)
    assert loss.dtype == torch.float32
    assert type(loss.grad_fn).__name__ == "_FusedXentBiasFnBackward"
    _close(loss, r_loss, 2e-4, "loss")
    loss.backward(dloss.cuda().view(()))
    assert xg.grad.dtype == torch.bfloat16 and bg.grad.dtype == torch.float32
    _close(xg.grad, r_dx, TOL[torch.bfloat16], "dx")
    _close(bg.grad, r_db, 2e-4, "dbias")
    # not the kernels' input: a 3-D tensor (classes in dimension 1), a CPU one
    x3, y3 = x.cuda().view(3, 3, 1031).transpose(1, 2), y.cuda().view(3, 3)
    for u, v, w in ((x3, y3, b.cuda()[:, None]), (x, y, b)):
        assert torch.equal(
            softmax_cross_entropy(u, v, 0.1, bias=w.flatten()),
            F.cross_entropy(u.float() + w, v, label_smoothing=0.1))


def test_native_entry_points_validate():
    core = _core()
    x, y = torch.randn(4, 64).cuda(), torch.zeros(4, dtype=torch.int64).cuda()
    b = torch.randn(64).cuda()
    lse, count = torch.zeros(4).cuda(), torch.ones(()).cuda()
    for bad in (b.bfloat16(), b[:63], b.cpu()):
        with pytest.raises(RuntimeError, match="bias"):
            core.fused_xent_bias_forward(x, bad, y, 0.0, IGNORE, "mean")
        with pytest.raises(RuntimeError, match="bias"):
            core.fused_xent_bias_backward(count, x, bad, y, lse, count, 0.0,
                                          IGNORE, "mean")


def _tiny_bert_losses(model, folded):
    from horovod_amd.models.bert import BertPretrainingLoss
    ids, types, labels, nsp = _bert_batch()
    labels = labels.clone()
    labels[:, ::5] = -100
    model.zero_grad()
    mlm, nsp_logits = model(ids, token_type_ids=types,
                            add_mlm_bias=not folded)
    loss = BertPretrainingLoss(fused=folded)(
        mlm, nsp_logits, labels, nsp,
        mlm_bias=model.mlm_bias if folded else None)
    loss.backward()
    return loss, {n: p.grad.clone() for n, p in model.named_parameters()}


def test_tiny_bert_loss_matches_stock():
    torch.manual_seed(0)
    model = _tiny_bert(True, 0.0).cuda().train()
    with torch.no_grad():
        model.mlm_bias.normal_()
    loss_s, grads_s = _tiny_bert_losses(model, False)
    loss_f, grads_f = _tiny_bert_losses(model, True)
    assert type(loss_f.grad_fn.next_functions[0][0]).__name__ == \
        "_FusedXentBiasFnBackward"
    _close(loss_f, loss_s.detach().double().cpu(), 2e-4, "loss")
    assert set(grads_f) == set(grads_s) and "mlm_bias" in grads_f
    for name, g in grads_f.items():
        _close(g, grads_s[name].double().cpu(), 2e-4, name)
