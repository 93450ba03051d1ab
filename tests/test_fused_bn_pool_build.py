"""The pooled stem path without a GPU: the bindings exist, forward_maxpool
falls back to the stock ops on CPU tensors, and the ResNet modules and
state_dict keys are what they were."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F


def test_bindings_exist():
    from horovod_amd import _core
    for name in ("fused_bn_relu_pool_forward", "fused_bn_relu_pool_backward",
                 "fused_bn_pool_pass", "fused_bn_pool_path"):
        assert callable(getattr(_core, name)), name
    assert isinstance(_core.fused_bn_pool_path(), bool)


def test_forward_maxpool_on_cpu_is_the_stock_ops():
    from horovod_amd.ops import FusedBNReLU
    torch.manual_seed(0)
    x = torch.randn(2, 8, 9, 10)
    for pool in (nn.MaxPool2d(3, stride=2, padding=1), nn.MaxPool2d(2, 2)):
        for training in (True, False):
            m = FusedBNReLU(8).train(training)
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
            stock = nn.BatchNorm2d(8).train(training)
            stock.load_state_dict(copy.deepcopy(m.state_dict()))
            xa = x.clone().requires_grad_(True)
            xb = x.clone().requires_grad_(True)
            got = m.forward_maxpool(xa, pool)
            exp = pool(F.relu(stock(xb)))
            assert torch.equal(got, exp)
            got.sum().backward()
            exp.sum().backward()
            assert torch.equal(xa.grad, xb.grad)
            assert torch.equal(m.weight.grad, stock.weight.grad)
            assert torch.equal(m.running_mean, stock.running_mean)
            assert torch.equal(m.running_var, stock.running_var)


def test_resnet_modules_and_state_dict_keys_unchanged(monkeypatch):
    from horovod_amd.models import resnet50
    from horovod_amd.ops import FusedBNAddReLU, FusedBNReLU
    monkeypatch.delenv("HOROVOD_FUSED_BN", raising=False)
    fused = resnet50(num_classes=10)
    stock = resnet50(num_classes=10, fused_bn=False)
    assert type(fused.bn1) is FusedBNReLU
    assert type(fused.maxpool) is nn.MaxPool2d
    assert {type(m) for m in fused.modules()
            if isinstance(m, nn.BatchNorm2d)} == \
        {FusedBNReLU, FusedBNAddReLU, nn.BatchNorm2d}
    assert [n for n, _ in fused.named_modules()] == \
        [n for n, _ in stock.named_modules()]
    assert list(fused.state_dict()) == list(stock.state_dict())
    assert {k: tuple(v.shape) for k, v in fused.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in stock.state_dict().items()}


def test_resnet_forward_goes_through_forward_maxpool(monkeypatch):
    """The fused model's stem calls bn1.forward_maxpool with its own maxpool
    module (which, on CPU, then runs it); the stock model does not."""
    from horovod_amd.models import resnet50
    from horovod_amd.ops import FusedBNReLU
    monkeypatch.delenv("HOROVOD_FUSED_BN", raising=False)
    calls = []
    real = FusedBNReLU.forward_maxpool

    def spy(self, input, pool):
        calls.append((self, pool))
        return real(self, input, pool)

    monkeypatch.setattr(FusedBNReLU, "forward_maxpool", spy)
    x = torch.randn(2, 3, 64, 64)
    fused = resnet50(num_classes=10).train()
    fused(x)
    assert len(calls) == 1
    assert calls[0][0] is fused.bn1 and calls[0][1] is fused.maxpool
    resnet50(num_classes=10, fused_bn=False).train()(x)
    assert len(calls) == 1
