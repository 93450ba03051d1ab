"""Fused softmax cross-entropy on the GPU against fp64: on CPU copies of the
already dtype-rounded logits, F.cross_entropy(x.double(), y, ...) with its
autograd gradient for a random incoming gradient, and torch.logsumexp.

|err| <= tol + tol * |ref| (_close).  loss, row loss and lse: 2e-4 in every
dtype, they are fp32 results of fp32 sums.  dx: fp32 2e-4, bf16 2^-8, fp16
2^-10, the figures of test_gpu_fused_gelu.py: the kernel rounds once from
fp32, half an ulp is at most 2^-9 |ref| in bf16 and 2^-11 |ref| in fp16.  For
these inputs the fp64 reference rounded once to the dtype reaches 0.46 (bf16)
and 0.21 (fp16) of the dx bound, and rounded to fp32 less than 3e-4 of any
2e-4 bound (checked on the CPU over the whole grid).

Grid: V {1, 2, 7, 8, 9, 1031, W, W + 1, 30522} x M {1, 9, 67}, W the longest
row that is given a wave (longer rows get a block).  1: softmax is 1; 7: head
only; 8, 9: one vector and a one-element tail; 1031: odd, all eight phases of
a 2-byte row start; 9 rows walk every phase and wrap, 67 is no multiple of the
rows of a block.  dtype, smoothing, reduction and "every third row ignored"
rotate by the rule in _grid().  Logits are 4 * randn with row 0 shifted by +50
and the last row by -50, so a missing max subtraction overflows.
"""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_fused_ln import _bert_batch, _close, _tiny_bert

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
REDUCTIONS = ["none", "mean", "sum"]
ROWS = [1, 9, 67]
TOL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
IGNORE = -100


def _core():
    from horovod_amd import _core
    return _core


def _vs():
    W = _core().fused_xent_wave_max_v()
    return [1, 2, 7, 8, 9, 1031, W, W + 1, 30522]


def _grid():
    cases = []
    for i, (M, V) in enumerate(itertools.product(ROWS, _vs())):
        r, c = divmod(i, 9)
        n = c + r
        cases.append((M, V, DTYPES[n % 3], 0.1 * (n % 2),
                      REDUCTIONS[(c + 2 * r) % 3], n // 2 % 2 == 1))
    # every dtype, reduction, smoothing and ignore choice with every V and M
    for key, vals in ((0, ROWS), (1, _vs())):
        for v in vals:
            sub = [c for c in cases if c[key] == v]
            assert {c[2] for c in sub} == set(DTYPES)
            assert {c[3] for c in sub} == {0.0, 0.1}
            assert {c[4] for c in sub} == set(REDUCTIONS)
            assert {c[5] for c in sub} == {True, False}
    return cases


def _id(case):
    M, V, dtype, eps, reduction, ignoring = case
    return (f"{M}x{V}-{str(dtype)[6:]}-eps{eps}-{reduction}-"
            f"{'ignore' if ignoring else 'all'}")


@functools.lru_cache(maxsize=None)
def _case(M, V, dtype, eps, reduction, ignoring):
    """dtype-rounded CPU inputs and the fp64 reference: (x, y, dloss), (loss,
    row loss, lse, dx)"""
    g = torch.Generator().manual_seed(7 * M + V)
    x = 4 * torch.randn(M, V, generator=g)
    x[0] += 50
    x[-1] -= 50
    x = x.to(dtype)
    y = torch.randint(0, V, (M,), generator=g)
    if ignoring:
        y[2::3] = IGNORE
    dloss = torch.randn(M if reduction == "none" else 1, generator=g)
    xd = x.double().requires_grad_(True)
    kw = dict(label_smoothing=eps, ignore_index=IGNORE)
    loss = F.cross_entropy(xd, y, reduction=reduction, **kw)
    dx, = torch.autograd.grad(loss, xd, dloss.double().view(loss.shape))
    rows = F.cross_entropy(xd, y, reduction="none", **kw).detach()
    return (x, y, dloss), (loss.detach(), rows,
                           torch.logsumexp(x.double(), 1), dx)


def _run_native(x, y, dloss, eps, reduction):
    core = _core()
    x, y = x.cuda(), y.cuda()
    out = core.fused_xent_forward(x, y, eps, IGNORE, reduction)
    loss, rows, lse, count = out
    dx = core.fused_xent_backward(dloss.cuda(), x, y, lse, count, eps, IGNORE,
                                  reduction)
    return loss, rows, lse, count, dx


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_matches_fp64_reference(case):
    M, V, dtype, eps, reduction, ignoring = case
    (x, y, dloss), (r_loss, r_rows, r_lse, r_dx) = _case(*case)
    loss, rows, lse, count, dx = _run_native(x, y, dloss, eps, reduction)
    assert loss.dtype == lse.dtype == count.dtype == torch.float32
    assert dx.dtype == dtype
    assert float(count) == int((y != IGNORE).sum())
    _close(loss, r_loss, 2e-4, "loss")
    if reduction == "none":
        assert rows is None
    else:
        _close(rows, r_rows, 2e-4, "row loss")
    _close(lse, r_lse, 2e-4, "lse")
    _close(dx, r_dx, TOL[dtype], "dx")
    if ignoring and M > 2:
        assert not bool(dx[2::3].any())


@pytest.mark.parametrize("M,V,dtype", [(67, 30522, torch.bfloat16),
                                       (9, 1031, torch.float32)])
def test_bitwise_reproducible(M, V, dtype):
    (x, y, dloss), _ = _case(M, V, dtype, 0.1, "mean", True)
    runs = [_run_native(x, y, dloss, 0.1, "mean") for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_all_rows_ignored():
    (x, _, dloss), _ = _case(9, 1031, torch.bfloat16, 0.1, "mean", True)
    y = torch.full((9,), IGNORE)
    loss, _, _, count, dx = _run_native(x, y, dloss, 0.1, "mean")
    assert bool(torch.isnan(loss)) and float(count) == 0
    assert not bool(dx.any())
    loss, _, _, _, dx = _run_native(x, y, dloss, 0.1, "sum")
    assert float(loss) == 0 and not bool(dx.any())


def test_label_out_of_range_poisons_its_row_only():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 9, generator=g)
    y = torch.tensor([9, 4, 0])
    dloss = torch.randn(3, generator=g)
    loss, _, _, _, dx = _run_native(x, y, dloss, 0.0, "none")
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(dx[0]).all())
    xd = x[1:].double().requires_grad_(True)
    ref = F.cross_entropy(xd, y[1:], reduction="none")
    _close(loss[1:], ref.detach(), 2e-4, "loss of the other rows")
    _close(dx[1:], torch.autograd.grad(ref, xd, dloss[1:].double())[0], 2e-4,
           "dx of the other rows")
    # the program goes on
    assert float(torch.ones(4, device="cuda").sum()) == 4


def test_public_function():
    from horovod_amd.ops import softmax_cross_entropy
    case = (9, 1031, torch.bfloat16, 0.1, "mean", True)
    (x, y, dloss), (r_loss, _, _, r_dx) = _case(*case)
    xg = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        loss = softmax_cross_entropy(xg, y.cuda(), 0.1, IGNORE, "mean")
    assert loss.dtype == torch.float32
    assert type(loss.grad_fn).__name__ == "_FusedXentFnBackward"
    _close(loss, r_loss, 2e-4, "loss")
    loss.backward(dloss.cuda().view(()))
    assert xg.grad.dtype == torch.bfloat16
    _close(xg.grad, r_dx, TOL[torch.bfloat16], "dx")
    # not the kernels' input: a 3-D tensor, a CPU tensor
    x3, y3 = x.cuda().view(3, 3, 1031).transpose(1, 2), y.cuda().view(3, 3)
    for a, b in ((x3, y3), (x, y)):
        assert torch.equal(softmax_cross_entropy(a, b, 0.1),
                           F.cross_entropy(a.float(), b, label_smoothing=0.1))


def test_native_entry_points_validate():
    core = _core()
    x, y = torch.randn(4, 64).cuda(), torch.zeros(4, dtype=torch.int64).cuda()
    lse, count = torch.zeros(4).cuda(), torch.ones(()).cuda()
    bad = [(x.cpu(), y, 0.0), (x, y.int(), 0.0),
           (torch.randn(64, 4).cuda().t(), y, 0.0),  # not contiguous
           (x, y[:3], 0.0), (x, y, 1.0)]
    for x_, y_, eps in bad:
        with pytest.raises(RuntimeError):
            core.fused_xent_forward(x_, y_, eps, IGNORE, "mean")
        with pytest.raises(RuntimeError):
            core.fused_xent_backward(count, x_, y_, lse, count, eps, IGNORE,
                                     "mean")


def _tiny_bert_losses(model, fused, autocast):
    from horovod_amd.models.bert import BertPretrainingLoss
    ids, types, labels, nsp = _bert_batch()
    labels = labels.clone()
    labels[:, ::5] = -100
    model.zero_grad()
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        mlm, nsp_logits = model(ids, token_type_ids=types)
        loss = BertPretrainingLoss(fused=fused)(mlm, nsp_logits, labels, nsp)
    loss.backward()
    return loss, {n: p.grad.clone() for n, p in model.named_parameters()}


def test_tiny_bert_loss_matches_stock():
    torch.manual_seed(0)
    model = _tiny_bert(True, 0.0).cuda().train()
    loss_s, grads_s = _tiny_bert_losses(model, False, False)
    loss_f, grads_f = _tiny_bert_losses(model, True, False)
    _close(loss_f, loss_s.detach().double().cpu(), 2e-4, "loss")
    for name, g in grads_f.items():
        _close(g, grads_s[name].double().cpu(), 2e-4, name)
    loss, _ = _tiny_bert_losses(model, True, True)
    assert bool(torch.isfinite(loss))
    mlm_term = loss.grad_fn.next_functions[0][0]
    assert type(mlm_term).__name__ == "_FusedXentFnBackward"
