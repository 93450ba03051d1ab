"""The ResNet models use the fused BatchNorm modules by default; on CPU
tensors those fall back to the stock ops, and HOROVOD_FUSED_BN=0 or a custom
norm_layer builds stock modules.  No GPU needed."""
import torch
import torch.nn as nn


def _bn_types(model):
    return {type(m) for m in model.modules() if isinstance(m, nn.BatchNorm2d)}


def test_default_matches_stock_on_cpu(monkeypatch):
    from horovod_amd.models import resnet50
    from horovod_amd.ops import FusedBNAddReLU, FusedBNReLU
    monkeypatch.delenv("HOROVOD_FUSED_BN", raising=False)
    torch.manual_seed(0)
    fused = resnet50(num_classes=10).train()
    stock = resnet50(num_classes=10, fused_bn=False).train()
    # the four downsample BNs have no ReLU behind them and stay stock
    assert _bn_types(fused) == {FusedBNReLU, FusedBNAddReLU, nn.BatchNorm2d}
    assert isinstance(fused.bn1, FusedBNReLU)
    assert _bn_types(stock) == {nn.BatchNorm2d}
    stock.load_state_dict(fused.state_dict())
    x = torch.randn(2, 3, 64, 64)
    out_f = fused(x)
    out_s = stock(x)
    assert torch.equal(out_f, out_s)
    out_f.sum().backward()
    out_s.sum().backward()
    for (name, pf), ps in zip(fused.named_parameters(), stock.parameters()):
        assert torch.equal(pf.grad, ps.grad), name
    for (name, bf), bs in zip(fused.named_buffers(), stock.buffers()):
        assert torch.equal(bf, bs), name


def test_env_and_norm_layer_turn_default_off(monkeypatch):
    from horovod_amd.models import resnet50
    from horovod_amd.ops import FusedBNReLU
    monkeypatch.setenv("HOROVOD_FUSED_BN", "0")
    assert _bn_types(resnet50(num_classes=10)) == {nn.BatchNorm2d}
    # an explicit argument wins over the environment
    assert isinstance(resnet50(num_classes=10, fused_bn=True).bn1, FusedBNReLU)
    monkeypatch.delenv("HOROVOD_FUSED_BN")

    class OtherNorm(nn.BatchNorm2d):
        pass

    assert _bn_types(resnet50(num_classes=10, norm_layer=OtherNorm)) == \
        {OtherNorm}
