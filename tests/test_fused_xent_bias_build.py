"""Fused softmax cross-entropy with a bias: the native surface exists after
build(), and on CPU tensors the public function is F.cross_entropy of logits +
bias, with bias=None today's result.  No GPU needed.
"""
import pytest
import torch
import torch.nn.functional as F


def test_core_symbols_and_cpu_tensors_raise():
    from horovod_amd import _core
    x, y = torch.randn(4, 64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_xent_bias_forward(x, torch.zeros(64), y, 0.0, -100, "mean")
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_xent_bias_backward(torch.ones(()), x, torch.zeros(64), y,
                                       torch.zeros(4), torch.ones(()), 0.0,
                                       -100, "mean")
    # 2048 rows of each of the 4 classes of a bf16 row of 30522
    assert 1 <= _core.fused_xent_bias_row_chunks(8192, 30522,
                                                 torch.bfloat16) <= 2048 // 16
    assert _core.fused_xent_bias_row_chunks(1, 7, torch.float32) == 1


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_equals_cross_entropy_of_the_sum_on_cpu(reduction):
    from horovod_amd.models.bert import BertPretrainingLoss
    from horovod_amd.ops import FusedCrossEntropyLoss, softmax_cross_entropy
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 37, generator=g, requires_grad=True)
    b = torch.randn(37, generator=g, requires_grad=True)
    y = torch.randint(0, 37, (12,), generator=g)
    y[::4] = -100
    kw = dict(reduction=reduction, label_smoothing=0.1)
    ref = F.cross_entropy(x + b, y, **kw)
    r_grads = torch.autograd.grad(ref.sum(), (x, b), retain_graph=True)
    mod = FusedCrossEntropyLoss(**kw)
    for out in (softmax_cross_entropy(x, y, bias=b, **kw), mod(x, y, b)):
        assert out.dtype == torch.float32 and torch.equal(out, ref)
        for got, want in zip(torch.autograd.grad(out.sum(), (x, b)), r_grads):
            assert torch.equal(got, want)
    # bias=None is the call without one
    assert torch.equal(softmax_cross_entropy(x, y, bias=None, **kw),
                       softmax_cross_entropy(x, y, **kw))
    # the BERT loss adds a bias it is given, fused or not
    nsp, nsp_y = torch.randn(2, 2, generator=g), torch.tensor([0, 1])
    ref = F.cross_entropy(x + b, y) + F.cross_entropy(nsp, nsp_y)
    for fused in (False, True):
        out = BertPretrainingLoss(fused)(x.view(2, 6, 37), nsp, y.view(2, 6),
                                         nsp_y, mlm_bias=b)
        assert torch.equal(out, ref)
