"""BERT-large for the pretraining benchmark config (BASELINE.json config 4:
"BERT-large pretrain with fp16 grad compression + tensor-fusion autotune").

Own compact implementation on torch built-ins: nn.TransformerEncoder layers
use scaled_dot_product_attention, which routes to the ROCm fused-attention
backends on MI355X; bf16 autocast covers the matmuls via hipBLASLt.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from horovod_amd.ops import FusedDropoutAddLayerNorm, FusedLayerNorm


class BertConfig:
    def __init__(self, vocab_size=30522, hidden=1024, layers=24, heads=16,
                 intermediate=4096, max_seq=512, type_vocab=2, dropout=0.1):
        self.vocab_size = vocab_size
        self.hidden = hidden
        self.layers = layers
        self.heads = heads
        self.intermediate = intermediate
        self.max_seq = max_seq
        self.type_vocab = type_vocab
        self.dropout = dropout


BERT_LARGE = BertConfig()
BERT_BASE = BertConfig(hidden=768, layers=12, heads=12, intermediate=3072)


def _fused_ln_default():
    return os.environ.get("HOROVOD_FUSED_LN", "0") == "1"


class FusedLNEncoderLayer(nn.Module):
    """Post-LN encoder layer with the parameters of nn.TransformerEncoderLayer
    (self_attn, linear1, linear2, norm1, norm2) whose two
    LayerNorm(residual + dropout(branch)) tails are one fused kernel each
    (horovod_amd.ops.FusedDropoutAddLayerNorm)."""

    def __init__(self, cfg):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(
            cfg.hidden, cfg.heads, dropout=cfg.dropout, batch_first=True)
        self.linear1 = nn.Linear(cfg.hidden, cfg.intermediate)
        self.dropout = nn.Dropout(cfg.dropout)
        self.linear2 = nn.Linear(cfg.intermediate, cfg.hidden)
        self.norm1 = FusedDropoutAddLayerNorm(cfg.hidden, p=cfg.dropout)
        self.norm2 = FusedDropoutAddLayerNorm(cfg.hidden, p=cfg.dropout)

    def _attention(self, x, key_padding_mask):
        """self_attn(x, x, x, need_weights=False) on self_attn's parameters,
        kept in [B, S, E] layout throughout.  nn.MultiheadAttention with
        batch_first works in [S, B, E] and hands back a transposed view,
        which norm1's kernel (contiguous rows) would not take; here out_proj
        sees [B, S, E], so its output is contiguous with no copy beyond the
        head merge that nn.MultiheadAttention makes too."""
        attn = self.self_attn
        b, s, e = x.shape
        qkv = F.linear(x, attn.in_proj_weight, attn.in_proj_bias)
        q, k, v = (t.view(b, s, attn.num_heads, attn.head_dim).transpose(1, 2)
                   for t in qkv.chunk(3, dim=-1))
        mask = None
        if key_padding_mask is not None:
            # True marks padding there, "may attend" here
            mask = ~key_padding_mask.bool()[:, None, None, :]
        o = F.scaled_dot_product_attention(
            q, k, v, attn_mask=mask,
            dropout_p=attn.dropout if self.training else 0.0)
        return attn.out_proj(o.transpose(1, 2).reshape(b, s, e))

    def forward(self, x, key_padding_mask=None):
        h = self.norm1(self._attention(x, key_padding_mask), x)
        return self.norm2(
            self.linear2(self.dropout(F.gelu(self.linear1(h)))), h)


class FusedLNEncoder(nn.Module):
    """A stack of FusedLNEncoderLayer under the parameter names of
    nn.TransformerEncoder (layers.N.*): state_dicts load strictly both
    ways."""

    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList(
            FusedLNEncoderLayer(cfg) for _ in range(cfg.layers))

    def forward(self, src, src_key_padding_mask=None):
        for layer in self.layers:
            src = layer(src, src_key_padding_mask)
        return src


class BertForPretraining(nn.Module):
    """Embeddings + encoder + tied MLM head + NSP head.

    fused_ln: build the encoder from FusedLNEncoderLayer and the other
    LayerNorms as FusedLayerNorm; None means on iff HOROVOD_FUSED_LN=1.  Off,
    the model is the stock nn.TransformerEncoder one.  Parameter names and
    shapes are the same either way.
    """

    def __init__(self, cfg=BERT_LARGE, fused_ln=None):
        super().__init__()
        self.cfg = cfg
        if fused_ln is None:
            fused_ln = _fused_ln_default()
        self.fused_ln = bool(fused_ln)
        layer_norm = FusedLayerNorm if self.fused_ln else nn.LayerNorm
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos_emb = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.type_emb = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.emb_norm = layer_norm(cfg.hidden)
        self.emb_drop = nn.Dropout(cfg.dropout)
        if self.fused_ln:
            self.encoder = FusedLNEncoder(cfg)
        else:
            layer = nn.TransformerEncoderLayer(
                d_model=cfg.hidden, nhead=cfg.heads,
                dim_feedforward=cfg.intermediate, dropout=cfg.dropout,
                activation="gelu", batch_first=True, norm_first=False)
            self.encoder = nn.TransformerEncoder(layer, cfg.layers,
                                                 enable_nested_tensor=False)
        self.mlm_transform = nn.Sequential(
            nn.Linear(cfg.hidden, cfg.hidden), nn.GELU(),
            layer_norm(cfg.hidden))
        self.mlm_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.nsp = nn.Linear(cfg.hidden, 2)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        b, s = input_ids.shape
        pos = torch.arange(s, device=input_ids.device).unsqueeze(0)
        x = self.tok_emb(input_ids) + self.pos_emb(pos)
        if token_type_ids is not None:
            x = x + self.type_emb(token_type_ids)
        x = self.emb_drop(self.emb_norm(x))
        pad_mask = None
        if attention_mask is not None:
            pad_mask = attention_mask == 0
        h = self.encoder(x, src_key_padding_mask=pad_mask)
        # tied MLM head (weight sharing with tok_emb, BERT-standard)
        mlm = self.mlm_transform(h) @ self.tok_emb.weight.t() + self.mlm_bias
        nsp = self.nsp(h[:, 0])
        return mlm, nsp


def bert_large(fused_ln=None):
    return BertForPretraining(BERT_LARGE, fused_ln=fused_ln)


def bert_base(fused_ln=None):
    return BertForPretraining(BERT_BASE, fused_ln=fused_ln)
