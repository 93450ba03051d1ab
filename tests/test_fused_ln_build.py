"""Fused dropout + add + LayerNorm: the native surface exists after build(),
the dropout mask function has the properties docs/api.md gives it (evaluated
on the host), the modules are drop-in for nn.LayerNorm on CPU tensors, and
the BERT model with fused_ln=True has the parameters of the stock one.  No
GPU needed.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

SEED, OFFSET = 0x1234_5678_9ABC_DEF0, 8


def _mask(rows, H, p, seed=SEED, offset=OFFSET):
    from horovod_amd import _core
    return _core.fused_ln_keep_mask(rows, H, p, seed, offset, "cpu")


def test_core_symbols_and_cpu_tensors_raise():
    from horovod_amd import _core
    for name in ("fused_ln_forward", "fused_ln_backward",
                 "fused_ln_keep_mask"):
        assert hasattr(_core, name), name
    x = torch.randn(4, 64)
    w, b = torch.ones(64), torch.zeros(64)
    x0, w0, b0 = x.clone(), w.clone(), b.clone()
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_ln_forward(x, None, w, b, 0.0, 1e-5, 0, 0, True)
    assert torch.equal(x, x0) and torch.equal(w, w0) and torch.equal(b, b0)


def test_host_mask_basics():
    m0 = _mask(5, 64, 0.0)
    assert m0.dtype == torch.uint8 and m0.shape == (5, 64)
    assert m0.device.type == "cpu"
    assert bool((m0 == 1).all())
    assert bool((_mask(5, 64, 1.0) == 0).all())
    a = _mask(16, 128, 0.5)
    assert set(a.unique().tolist()) == {0, 1}
    assert torch.equal(a, _mask(16, 128, 0.5))
    assert not torch.equal(a, _mask(16, 128, 0.5, seed=SEED + 1))
    assert not torch.equal(a, _mask(16, 128, 0.5, offset=OFFSET + 4))
    # the high halves of seed and offset count too
    assert not torch.equal(a, _mask(16, 128, 0.5, seed=SEED ^ (1 << 40)))
    assert not torch.equal(a, _mask(16, 128, 0.5, offset=OFFSET + (1 << 32)))


def test_host_mask_known_answer():
    """Philox4x32-10 of counter 0 under key 0 is 6627e8d5 e169c58d bc57ac4c
    9b00dbd8 (the Random123 known-answer vector); elements take its 16-bit
    halves, low half first, and are kept iff the value >= round(p * 65536)."""
    vals = [0xe8d5, 0x6627, 0xc58d, 0xe169, 0xac4c, 0xbc57, 0xdbd8, 0x9b00]
    for t16 in (0x6627, 0x6628, 0x9b00, 0x9b01, 0xe8d5, 0xe8d6):
        m = _mask(1, 8, t16 / 65536.0, seed=0, offset=0)
        assert m[0].tolist() == [int(v >= t16) for v in vals], hex(t16)


def test_host_mask_rows_are_a_prefix():
    assert torch.equal(_mask(3, 64, 0.3), _mask(7, 64, 0.3)[:3])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_host_mask_keep_counts(p):
    rows, H = 64, 1024
    m = _mask(rows, H, p).to(torch.int64)
    t16 = round(p * 65536)
    q = 1.0 - t16 / 65536.0  # the keep probability after quantisation

    def check(count, n, what):
        sd = math.sqrt(n * q * (1.0 - q))
        assert abs(count - n * q) <= 5.0 * sd, (what, count, n * q, sd)

    check(int(m.sum()), rows * H, "all")
    for c, count in enumerate(m.sum(0).tolist()):
        check(count, rows, f"column {c}")
    per_pos = m.view(rows, H // 8, 8).sum((0, 1)).tolist()
    for k, count in enumerate(per_pos):
        check(count, rows * H // 8, f"position {k}")


def test_bad_arguments_raise():
    from horovod_amd import _core
    from horovod_amd.ops import (FusedDropoutAddLayerNorm,
                                 dropout_add_layer_norm)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError):
            FusedDropoutAddLayerNorm(64, p=p)
        with pytest.raises(ValueError):
            dropout_add_layer_norm(torch.randn(2, 64), None, None, None, p)
        with pytest.raises(RuntimeError):
            _core.fused_ln_keep_mask(2, 64, p, 0, 0, "cpu")
    with pytest.raises(RuntimeError):
        _core.fused_ln_keep_mask(2, 12, 0.5, 0, 0, "cpu")


@pytest.mark.parametrize("training", [False, True])
def test_modules_equal_composite_on_cpu(training):
    from horovod_amd.ops import FusedDropoutAddLayerNorm, FusedLayerNorm
    torch.manual_seed(3)
    stock = nn.LayerNorm(64)
    with torch.no_grad():
        stock.weight.uniform_(0.5, 1.5)
        stock.bias.uniform_(-0.5, 0.5)
    # eval mode with dropout configured, and training with p = 0
    fused = FusedDropoutAddLayerNorm(64, p=0.0 if training else 0.3)
    plain = FusedLayerNorm(64)
    fused.load_state_dict(stock.state_dict())
    plain.load_state_dict(stock.state_dict())
    for mod in (stock, fused, plain):
        mod.train(training)
    x = torch.randn(5, 7, 64, requires_grad=True)
    r = torch.randn(5, 7, 64, requires_grad=True)
    ref = stock(r + F.dropout(x, fused.p, training))
    out = fused(x, r)
    assert torch.equal(out, ref)
    assert torch.equal(plain(x), stock(x))
    assert torch.equal(fused(x), stock(x))
    gx, gr, gw = torch.autograd.grad(ref.square().sum(),
                                     [x, r, stock.weight])
    fx, fr, fw = torch.autograd.grad(out.square().sum(),
                                     [x, r, fused.weight])
    assert torch.equal(fx, gx) and torch.equal(fr, gr) and torch.equal(fw, gw)


def test_state_dict_round_trip():
    from horovod_amd.ops import FusedDropoutAddLayerNorm, FusedLayerNorm
    stock = nn.LayerNorm(32)
    with torch.no_grad():
        stock.weight.normal_()
        stock.bias.normal_()
    for mod in (FusedLayerNorm(32), FusedDropoutAddLayerNorm(32, p=0.1)):
        assert set(mod.state_dict()) == set(stock.state_dict())
        mod.load_state_dict(stock.state_dict(), strict=True)
        assert torch.equal(mod.weight, stock.weight)
        back = nn.LayerNorm(32)
        back.load_state_dict(mod.state_dict(), strict=True)
        assert torch.equal(back.bias, stock.bias)
    assert FusedDropoutAddLayerNorm(32, p=0.25).p == 0.25
    assert FusedDropoutAddLayerNorm(32).p == 0.0


def _tiny_cfg(dropout=0.1):
    from horovod_amd.models.bert import BertConfig
    return BertConfig(vocab_size=100, hidden=64, layers=2, heads=4,
                      intermediate=128, max_seq=16, dropout=dropout)


def test_tiny_bert_fused_matches_stock_on_cpu():
    from horovod_amd.models.bert import BertForPretraining
    from horovod_amd.ops import FusedDropoutAddLayerNorm, FusedLayerNorm
    torch.manual_seed(0)
    stock = BertForPretraining(_tiny_cfg(), fused_ln=False)
    fused = BertForPretraining(_tiny_cfg(), fused_ln=True)
    assert isinstance(stock.encoder, nn.TransformerEncoder)
    assert not isinstance(fused.encoder, nn.TransformerEncoder)
    assert isinstance(fused.emb_norm, FusedLayerNorm)
    assert isinstance(fused.mlm_transform[2], FusedLayerNorm)
    for layer in fused.encoder.layers:
        assert isinstance(layer.norm1, FusedDropoutAddLayerNorm)
        assert isinstance(layer.norm2, FusedDropoutAddLayerNorm)
        assert layer.norm1.p == layer.norm2.p == 0.1
    sd_s, sd_f = stock.state_dict(), fused.state_dict()
    assert list(sd_s) == list(sd_f)
    assert "encoder.layers.1.self_attn.in_proj_weight" in sd_f
    for k in sd_s:
        assert sd_s[k].shape == sd_f[k].shape, k
    # strict loading both ways
    other = BertForPretraining(_tiny_cfg(), fused_ln=False)
    other.load_state_dict(sd_f, strict=True)
    fused.load_state_dict(sd_s, strict=True)
    stock.eval()
    fused.eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 100, (4, 16), generator=g)
    types = torch.randint(0, 2, (4, 16), generator=g)
    attn = torch.ones(4, 16, dtype=torch.long)
    attn[1, 11:] = 0
    for kw in (dict(), dict(token_type_ids=types, attention_mask=attn)):
        mlm_s, nsp_s = stock(ids, **kw)
        mlm_f, nsp_f = fused(ids, **kw)
        torch.testing.assert_close(mlm_f, mlm_s, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(nsp_f, nsp_s, rtol=2e-4, atol=2e-4)


def test_fused_layer_attention_is_contiguous_and_matches_mha():
    """the fused layer applies self_attn's parameters in [B, S, E] layout, so
    norm1 gets contiguous rows; nn.MultiheadAttention(batch_first=True)
    returns a transposed view"""
    from horovod_amd.models.bert import FusedLNEncoderLayer
    torch.manual_seed(2)
    layer = FusedLNEncoderLayer(_tiny_cfg()).eval()
    x = torch.randn(4, 16, 64)
    pad = torch.zeros(4, 16, dtype=torch.bool)
    pad[1, 11:] = True
    pad[3, 5:] = True
    for kpm in (None, pad):
        ref = layer.self_attn(x, x, x, key_padding_mask=kpm,
                              need_weights=False)[0]
        out = layer._attention(x, kpm)
        assert out.shape == (4, 16, 64) and out.is_contiguous()
        torch.testing.assert_close(out, ref, rtol=2e-4, atol=2e-4)
        g_ref, = torch.autograd.grad(ref.square().sum(),
                                     layer.self_attn.in_proj_weight)
        g_out, = torch.autograd.grad(out.square().sum(),
                                     layer.self_attn.in_proj_weight)
        torch.testing.assert_close(g_out, g_ref, rtol=2e-4, atol=2e-4)


def test_env_resolution(monkeypatch):
    from horovod_amd.models import bert
    monkeypatch.delenv("HOROVOD_FUSED_LN", raising=False)
    assert isinstance(bert.BertForPretraining(_tiny_cfg()).encoder,
                      nn.TransformerEncoder)
    monkeypatch.setenv("HOROVOD_FUSED_LN", "1")
    assert isinstance(bert.BertForPretraining(_tiny_cfg()).encoder,
                      bert.FusedLNEncoder)
    # an explicit argument wins over the environment
    assert isinstance(
        bert.BertForPretraining(_tiny_cfg(), fused_ln=False).encoder,
        nn.TransformerEncoder)
    monkeypatch.setenv("HOROVOD_FUSED_LN", "0")
    assert isinstance(bert.BertForPretraining(_tiny_cfg()).encoder,
                      nn.TransformerEncoder)
    assert isinstance(
        bert.BertForPretraining(_tiny_cfg(), fused_ln=True).encoder,
        bert.FusedLNEncoder)
    # the factories pass the argument on (signature only: the real models
    # are too large to build here)
    import inspect
    for fn in (bert.bert_base, bert.bert_large):
        assert "fused_ln" in inspect.signature(fn).parameters
