"""Fused self-attention: the native surface exists after build(), input the
kernels do not take goes through the composite and equals SDPA, bad arguments
raise, and the BERT model resolves fused_attn like fused_gelu.  No GPU needed.
"""
import inspect

import pytest
import torch
import torch.nn.functional as F


def _sdpa(qkv, heads, pad):
    b, s, e3 = qkv.shape
    q, k, v = (t.view(b, s, heads, e3 // 3 // heads).transpose(1, 2)
               for t in qkv.chunk(3, dim=-1))
    mask = None if pad is None else ~pad[:, None, None, :]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    return o.transpose(1, 2).reshape(b, s, e3 // 3)


def test_core_symbols_and_cpu_tensors_raise():
    from horovod_amd import _core
    qkv = torch.randn(2, 8, 384).bfloat16()
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_attention_forward(qkv, None, 2, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_attention_backward(qkv[..., :128].contiguous(), qkv,
                                       qkv[..., :128].contiguous(),
                                       torch.zeros(2, 2, 8), None, 2, 0.0, 0, 0)


# CPU tensors at a covered shape, head dimension 32, S = 513
@pytest.mark.parametrize("S,heads,E", [(24, 2, 128), (24, 4, 128),
                                       (513, 1, 64)])
def test_uncovered_input_takes_the_composite(S, heads, E):
    from horovod_amd.ops import self_attention
    g = torch.Generator().manual_seed(S + heads)
    qkv = torch.randn(2, S, 3 * E, generator=g, requires_grad=True)
    pad = torch.arange(S)[None, :] >= torch.tensor([S, S // 3])[:, None]
    for mask in (None, pad):
        # eval mode with dropout configured, and training with p = 0
        for p, training in ((0.3, False), (0.0, True)):
            got = self_attention(qkv, heads, mask, p, training)
            want = _sdpa(qkv, heads, mask)
            assert torch.equal(got, want)
            assert torch.equal(torch.autograd.grad(got.square().sum(), qkv)[0],
                               torch.autograd.grad(want.square().sum(), qkv)[0])


def test_bad_arguments_raise():
    from horovod_amd.ops import self_attention
    qkv = torch.randn(2, 8, 384)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError):
            self_attention(qkv, 2, None, p)
    with pytest.raises(ValueError):
        self_attention(qkv, 5)
    with pytest.raises(ValueError):
        self_attention(qkv[0], 2)


def test_env_resolution(monkeypatch):
    from horovod_amd.models import bert
    cfg = bert.BertConfig(vocab_size=100, hidden=128, layers=2, heads=2,
                          intermediate=256, max_seq=16, dropout=0.1)

    def on(**kw):
        m = bert.BertForPretraining(cfg, **kw)
        layers = m.encoder.layers
        assert m.fused_attn == all(getattr(l, "fused_attn", False)
                                   for l in layers)
        return m.fused_attn

    for var in ("HOROVOD_FUSED_LN", "HOROVOD_FUSED_GELU", "HOROVOD_FUSED_ATTN"):
        monkeypatch.delenv(var, raising=False)
    # unset: the present model, stock or fused LayerNorm
    assert not on() and not on(fused_ln=True)
    assert type(bert.BertForPretraining(cfg).encoder) is \
        torch.nn.TransformerEncoder
    assert on(fused_ln=True, fused_attn=True)
    with pytest.raises(ValueError, match="fused_attn needs fused_ln"):
        on(fused_attn=True)
    monkeypatch.setenv("HOROVOD_FUSED_ATTN", "1")
    with pytest.raises(ValueError):
        on()
    assert on(fused_ln=True)
    # an explicit argument wins over the environment
    assert not on(fused_ln=True, fused_attn=False)
    for fn in (bert.bert_base, bert.bert_large):
        assert "fused_attn" in inspect.signature(fn).parameters


def test_bert_state_dict_and_eval_output_do_not_change():
    from horovod_amd.models import bert
    cfg = bert.BertConfig(vocab_size=100, hidden=128, layers=2, heads=2,
                          intermediate=256, max_seq=16, dropout=0.1)
    torch.manual_seed(0)
    off = bert.BertForPretraining(cfg, fused_ln=True, fused_attn=False).eval()
    on = bert.BertForPretraining(cfg, fused_ln=True, fused_attn=True).eval()
    assert list(on.state_dict()) == list(off.state_dict())
    on.load_state_dict(off.state_dict(), strict=True)
    off.load_state_dict(on.state_dict(), strict=True)
    ids = torch.randint(0, 100, (4, 16),
                        generator=torch.Generator().manual_seed(1))
    attn = torch.ones(4, 16, dtype=torch.long)
    attn[1, 5:] = 0
    # on CPU tensors the fused layer is the composite: the same numbers
    for a, b in zip(on(ids, attention_mask=attn), off(ids, attention_mask=attn)):
        assert torch.equal(a, b)
