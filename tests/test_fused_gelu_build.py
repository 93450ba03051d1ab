"""Fused bias + GELU + dropout: the native surface exists after build(), the
function and the module are the composite on CPU tensors, FusedLinearGELU is
state_dict-compatible with nn.Linear, and the BERT model has the same keys
with fused_gelu on.  No GPU needed.
"""
import inspect

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def test_core_symbols_and_cpu_tensors_raise():
    from horovod_amd import _core
    x, b = torch.randn(4, 64), torch.randn(64)
    x0, b0 = x.clone(), b.clone()
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_bias_gelu_forward(x, b, 0.0, 0, 0, False)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_bias_gelu_backward(x, x, b, 0.0, 0, 0, False, True)
    assert torch.equal(x, x0) and torch.equal(b, b0)


@pytest.mark.parametrize("approximate", ["none", "tanh"])
@pytest.mark.parametrize("training", [False, True])
def test_equals_composite_on_cpu(training, approximate):
    from horovod_amd.ops import FusedLinearGELU, bias_gelu_dropout
    torch.manual_seed(3)
    # eval mode with dropout configured, and training with p = 0
    p = 0.0 if training else 0.3
    stock = nn.Linear(24, 40)
    mod = FusedLinearGELU(24, 40, p=p, approximate=approximate)
    mod.load_state_dict(stock.state_dict())
    mod.train(training)
    x = torch.randn(5, 7, 24, requires_grad=True)
    ref = F.dropout(F.gelu(stock(x), approximate=approximate), p, training)
    out = mod(x)
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)
    g_ref = torch.autograd.grad(ref.square().sum(), [x, *stock.parameters()])
    g_out = torch.autograd.grad(out.square().sum(), [x, *mod.parameters()])
    for a, b in zip(g_out, g_ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    u = torch.randn(5, 40, requires_grad=True)
    for bias in (stock.bias, None):
        got = bias_gelu_dropout(u, bias, p, training, approximate)
        want = F.gelu(u if bias is None else u + bias, approximate=approximate)
        assert torch.equal(got, want)
        assert torch.equal(torch.autograd.grad(got.sum(), u)[0],
                           torch.autograd.grad(want.sum(), u)[0])


def test_bad_arguments_raise():
    from horovod_amd.ops import FusedLinearGELU, bias_gelu_dropout
    x = torch.randn(2, 8)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError):
            bias_gelu_dropout(x, None, p)
        with pytest.raises(ValueError):
            FusedLinearGELU(8, 8, p=p)
    with pytest.raises(ValueError):
        bias_gelu_dropout(x, None, 0.0, True, "erf")
    with pytest.raises(ValueError):
        FusedLinearGELU(8, 8, approximate="fast")


def test_state_dict_round_trip_with_linear():
    from horovod_amd.ops import FusedLinearGELU
    stock = nn.Linear(16, 32)
    mod = FusedLinearGELU(16, 32, p=0.1, approximate="tanh")
    assert list(mod.state_dict()) == list(stock.state_dict())
    mod.load_state_dict(stock.state_dict(), strict=True)
    back = nn.Linear(16, 32)
    back.load_state_dict(mod.state_dict(), strict=True)
    assert torch.equal(back.weight, stock.weight)
    assert torch.equal(back.bias, stock.bias)
    assert (mod.p, mod.approximate) == (0.1, "tanh")
    assert list(FusedLinearGELU(16, 32, bias=False).state_dict()) == ["weight"]


def _tiny_cfg():
    from horovod_amd.models.bert import BertConfig
    return BertConfig(vocab_size=100, hidden=64, layers=2, heads=4,
                      intermediate=128, max_seq=16, dropout=0.1)


def test_bert_keys_are_the_same_in_all_three_configurations():
    from horovod_amd.models.bert import BertForPretraining
    from horovod_amd.ops import FusedLinearGELU
    torch.manual_seed(0)
    models = [BertForPretraining(_tiny_cfg(), fused_ln=ln, fused_gelu=gelu)
              for ln, gelu in ((False, False), (True, False), (True, True))]
    full = models[2]
    assert isinstance(full.mlm_transform[0], FusedLinearGELU)
    assert full.mlm_transform[0].p == 0.0
    assert isinstance(full.mlm_transform[1], nn.Identity)
    for layer in full.encoder.layers:
        assert isinstance(layer.linear1, FusedLinearGELU)
        assert layer.linear1.p == 0.1
    assert type(models[1].encoder.layers[0].linear1) is nn.Linear
    assert type(models[1].mlm_transform[1]) is nn.GELU
    sds = [m.state_dict() for m in models]
    for sd in sds[1:]:
        assert list(sd) == list(sds[0])
        assert [v.shape for v in sd.values()] == \
            [v.shape for v in sds[0].values()]
    for m in models:
        for sd in sds:
            m.load_state_dict(sd, strict=True)
    # one set of weights, eval mode: the three models agree
    ids = torch.randint(0, 100, (4, 16),
                        generator=torch.Generator().manual_seed(1))
    outs = [m.eval()(ids) for m in models]
    for mlm, nsp in outs[1:]:
        torch.testing.assert_close(mlm, outs[0][0], rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(nsp, outs[0][1], rtol=2e-4, atol=2e-4)


def test_env_resolution(monkeypatch):
    from horovod_amd.models import bert
    from horovod_amd.ops import FusedLinearGELU

    def on(**kw):
        m = bert.BertForPretraining(_tiny_cfg(), **kw)
        return isinstance(m.mlm_transform[0], FusedLinearGELU)

    monkeypatch.delenv("HOROVOD_FUSED_LN", raising=False)
    monkeypatch.delenv("HOROVOD_FUSED_GELU", raising=False)
    assert not on() and not on(fused_ln=True)
    assert on(fused_ln=True, fused_gelu=True)
    with pytest.raises(ValueError):
        on(fused_gelu=True)
    monkeypatch.setenv("HOROVOD_FUSED_GELU", "1")
    with pytest.raises(ValueError):
        on()
    assert on(fused_ln=True)
    # an explicit argument wins over the environment
    assert not on(fused_ln=True, fused_gelu=False)
    assert not on(fused_gelu=False)
    monkeypatch.setenv("HOROVOD_FUSED_LN", "1")
    assert on()
    monkeypatch.setenv("HOROVOD_FUSED_GELU", "0")
    assert not on()
    for fn in (bert.bert_base, bert.bert_large):
        assert "fused_gelu" in inspect.signature(fn).parameters
