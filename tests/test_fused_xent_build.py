"""Fused softmax cross-entropy: the native surface exists after build(), the
function and the module are F.cross_entropy on CPU tensors, bad arguments
raise, and BertPretrainingLoss resolves HOROVOD_FUSED_XENT.  No GPU needed.
"""
import pytest
import torch
import torch.nn.functional as F


def test_core_symbols_and_cpu_tensors_raise():
    from horovod_amd import _core
    x, y = torch.randn(4, 64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_xent_forward(x, y, 0.0, -100, "mean")
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_xent_backward(torch.ones(()), x, y, torch.zeros(4),
                                  torch.ones(()), 0.0, -100, "mean")
    assert _core.fused_xent_wave_max_v() >= 8


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_equals_cross_entropy_on_cpu(reduction):
    from horovod_amd.ops import FusedCrossEntropyLoss, softmax_cross_entropy
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 37, generator=g, requires_grad=True)
    y = torch.randint(0, 37, (12,), generator=g)
    y[::4] = -1
    ref = F.cross_entropy(x, y, ignore_index=-1, reduction=reduction,
                          label_smoothing=0.1)
    mod = FusedCrossEntropyLoss(label_smoothing=0.1, ignore_index=-1,
                                reduction=reduction)
    for out in (softmax_cross_entropy(x, y, 0.1, -1, reduction), mod(x, y)):
        assert out.dtype == torch.float32 and torch.equal(out, ref)
        assert torch.equal(torch.autograd.grad(out.sum(), x)[0],
                           torch.autograd.grad(ref.sum(), x,
                                               retain_graph=True)[0])
    # fp32 loss for bf16 logits too
    out = softmax_cross_entropy(x.detach().bfloat16(), y, 0.1, -1, reduction)
    assert out.dtype == torch.float32


def test_bad_arguments_raise():
    from horovod_amd.ops import FusedCrossEntropyLoss, softmax_cross_entropy
    x, y = torch.randn(2, 8), torch.zeros(2, dtype=torch.int64)
    for kw in ({"label_smoothing": 1.0}, {"label_smoothing": -0.1},
               {"reduction": "batchmean"}):
        with pytest.raises(ValueError):
            softmax_cross_entropy(x, y, **kw)
        with pytest.raises(ValueError):
            FusedCrossEntropyLoss(**kw)
    with pytest.raises(TypeError):
        FusedCrossEntropyLoss(weight=torch.ones(8))


def test_env_resolution(monkeypatch):
    from horovod_amd.models.bert import BertPretrainingLoss
    monkeypatch.delenv("HOROVOD_FUSED_XENT", raising=False)
    assert not BertPretrainingLoss().fused
    assert BertPretrainingLoss(fused=True).fused
    monkeypatch.setenv("HOROVOD_FUSED_XENT", "1")
    built = BertPretrainingLoss()
    assert built.fused and not BertPretrainingLoss(fused=False).fused
    # read when the module is built
    monkeypatch.setenv("HOROVOD_FUSED_XENT", "0")
    assert built.fused and not BertPretrainingLoss().fused
    # both settings are the two F.cross_entropy calls on CPU tensors
    g = torch.Generator().manual_seed(1)
    mlm, nsp = torch.randn(2, 5, 11, generator=g), torch.randn(2, 2, generator=g)
    labels = torch.randint(0, 11, (2, 5), generator=g)
    labels[0, 1] = -100
    nsp_y = torch.tensor([0, 1])
    ref = (F.cross_entropy(mlm.view(-1, 11), labels.view(-1)) +
           F.cross_entropy(nsp, nsp_y))
    for fused in (False, True):
        out = BertPretrainingLoss(fused)(mlm, nsp, labels, nsp_y)
        assert torch.equal(out, ref)
