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

from horovod_amd.ops import (FusedDropoutAddLayerNorm, FusedLayerNorm,
                             FusedLinearGELU, embedding_layer_norm,
                             gather_labelled_rows, self_attention,
                             softmax_cross_entropy)


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


def _fused_gelu_default():
    return os.environ.get("HOROVOD_FUSED_GELU", "0") == "1"


def _fused_attn_default():
    return os.environ.get("HOROVOD_FUSED_ATTN", "0") == "1"


def _fused_emb_default():
    return os.environ.get("HOROVOD_FUSED_EMB", "0") == "1"


def _fused_xent_default():
    return os.environ.get("HOROVOD_FUSED_XENT", "0") == "1"


class FusedLNEncoderLayer(nn.Module):
    """Post-LN encoder layer with the parameters of nn.TransformerEncoderLayer
    (self_attn, linear1, linear2, norm1, norm2) whose two
    LayerNorm(residual + dropout(branch)) tails are one fused kernel each
    (horovod_amd.ops.FusedDropoutAddLayerNorm).  With fused_gelu, linear1 is
    a FusedLinearGELU that also applies the GELU and the dropout behind
    it.  With fused_attn, the attention core between in_proj and out_proj is
    horovod_amd.ops.self_attention on the packed in_proj output; self_attn
    still holds the parameters."""

    def __init__(self, cfg, fused_gelu=False, fused_attn=False):
        super().__init__()
        self.fused_gelu = fused_gelu
        self.fused_attn = fused_attn
        self.self_attn = nn.MultiheadAttention(
            cfg.hidden, cfg.heads, dropout=cfg.dropout, batch_first=True)
        if fused_gelu:
            self.linear1 = FusedLinearGELU(cfg.hidden, cfg.intermediate,
                                           p=cfg.dropout)
        else:
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
        if self.fused_attn:
            mask = key_padding_mask
            if mask is not None and mask.dtype != torch.bool:
                mask = mask.bool()
            return attn.out_proj(self_attention(
                qkv, attn.num_heads, mask, attn.dropout, self.training))
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
        if self.fused_gelu:
            return self.norm2(self.linear2(self.linear1(h)), h)
        return self.norm2(
            self.linear2(self.dropout(F.gelu(self.linear1(h)))), h)


class FusedLNEncoder(nn.Module):
    """A stack of FusedLNEncoderLayer under the parameter names of
    nn.TransformerEncoder (layers.N.*): state_dicts load strictly both
    ways."""

    def __init__(self, cfg, fused_gelu=False, fused_attn=False):
        super().__init__()
        self.layers = nn.ModuleList(
            FusedLNEncoderLayer(cfg, fused_gelu, fused_attn)
            for _ in range(cfg.layers))

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

    fused_gelu: on top of fused_ln, every encoder layer's linear1 and the MLM
    head's Linear are FusedLinearGELU (bias + GELU + dropout in one kernel
    pass); None means on iff HOROVOD_FUSED_GELU=1.  It needs fused_ln: the
    stock nn.TransformerEncoder has no place for the fused feed-forward.

    fused_attn: on top of fused_ln, every encoder layer's attention core runs
    on the project's matrix-instruction kernels
    (horovod_amd.ops.self_attention); None means on iff HOROVOD_FUSED_ATTN=1.
    It needs fused_ln for the same reason.  A sequence whose keys are all
    padding then gets zeros from the attention, not NaN.

    fused_emb: on top of fused_ln, the three embedding lookups, emb_norm and
    emb_drop run as one kernel pass (horovod_amd.ops.embedding_layer_norm) on
    the parameters of those modules, and hand the encoder its activations in
    the autocast dtype; None means on iff HOROVOD_FUSED_EMB=1.  It needs
    fused_ln for the same reason.
    """

    def __init__(self, cfg=BERT_LARGE, fused_ln=None, fused_gelu=None,
                 fused_attn=None, fused_emb=None):
        super().__init__()
        self.cfg = cfg
        if fused_ln is None:
            fused_ln = _fused_ln_default()
        if fused_gelu is None:
            fused_gelu = _fused_gelu_default()
        if fused_attn is None:
            fused_attn = _fused_attn_default()
        if fused_emb is None:
            fused_emb = _fused_emb_default()
        self.fused_ln = bool(fused_ln)
        self.fused_gelu = bool(fused_gelu)
        self.fused_attn = bool(fused_attn)
        self.fused_emb = bool(fused_emb)
        if self.fused_emb and not self.fused_ln:
            raise ValueError("fused_emb needs fused_ln: it hands the encoder "
                             "activations in the autocast dtype")
        if self.fused_gelu and not self.fused_ln:
            raise ValueError("fused_gelu needs fused_ln: the stock encoder "
                             "has no place for the fused feed-forward")
        if self.fused_attn and not self.fused_ln:
            raise ValueError("fused_attn needs fused_ln: the stock encoder "
                             "has no place for the fused attention")
        layer_norm = FusedLayerNorm if self.fused_ln else nn.LayerNorm
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos_emb = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.type_emb = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.emb_norm = layer_norm(cfg.hidden)
        self.emb_drop = nn.Dropout(cfg.dropout)
        if self.fused_ln:
            self.encoder = FusedLNEncoder(cfg, self.fused_gelu,
                                          self.fused_attn)
        else:
            layer = nn.TransformerEncoderLayer(
                d_model=cfg.hidden, nhead=cfg.heads,
                dim_feedforward=cfg.intermediate, dropout=cfg.dropout,
                activation="gelu", batch_first=True, norm_first=False)
            self.encoder = nn.TransformerEncoder(layer, cfg.layers,
                                                 enable_nested_tensor=False)
        if self.fused_gelu:
            # the same indices and key names: the GELU moves into module 0
            self.mlm_transform = nn.Sequential(
                FusedLinearGELU(cfg.hidden, cfg.hidden, p=0.0), nn.Identity(),
                layer_norm(cfg.hidden))
        else:
            self.mlm_transform = nn.Sequential(
                nn.Linear(cfg.hidden, cfg.hidden), nn.GELU(),
                layer_norm(cfg.hidden))
        self.mlm_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.nsp = nn.Linear(cfg.hidden, 2)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None,
                add_mlm_bias=True, mlm_labels=None, max_predictions=None):
        """add_mlm_bias=False returns the MLM logits as the vocabulary GEMM
        leaves them (bf16 under autocast), for a loss that adds mlm_bias
        itself: BertPretrainingLoss(fused=True)(..., mlm_bias=model.mlm_bias).

        mlm_labels [B, S]: the MLM head runs on the labelled positions only
        (label != -100, horovod_amd.ops.gather_labelled_rows) and the call
        returns (mlm_logits [capacity, V], nsp_logits, row_labels [capacity])
        for BertPretrainingLoss(mlm_logits, nsp_logits, row_labels, ...).
        capacity is B * max_predictions, with nothing read on the host; more
        labelled positions than that in a batch make the logits NaN.  Without
        max_predictions the count is read on the host."""
        if self.fused_emb:
            x = embedding_layer_norm(
                input_ids, token_type_ids, self.tok_emb.weight,
                self.pos_emb.weight, self.type_emb.weight,
                self.emb_norm.weight, self.emb_norm.bias, self.emb_drop.p,
                self.emb_norm.eps, self.training)
        else:
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
        rows, row_labels = h, None
        if mlm_labels is not None:
            capacity = None
            if max_predictions is not None:
                capacity = h.shape[0] * max_predictions
            rows, row_labels = gather_labelled_rows(h, mlm_labels, capacity)
        # tied MLM head (weight sharing with tok_emb, BERT-standard)
        mlm = self.mlm_transform(rows) @ self.tok_emb.weight.t()
        if add_mlm_bias:
            mlm = mlm + self.mlm_bias
        nsp = self.nsp(h[:, 0])
        if mlm_labels is not None:
            return mlm, nsp, row_labels
        return mlm, nsp


class BertPretrainingLoss(nn.Module):
    """The pretraining loss of BertForPretraining's two outputs: the MLM
    cross-entropy over mlm_logits.flatten(0, 1), where a label of -100 marks a
    position that was not masked, plus the NSP cross-entropy.  mlm_logits
    [rows, V] with mlm_labels [rows], as a model called with mlm_labels
    returns them, are taken as they are.

    fused: take the MLM term through horovod_amd.ops.softmax_cross_entropy,
    which reads the [B * S, V] logits in their own dtype instead of an fp32
    copy; None means on iff HOROVOD_FUSED_XENT=1, read when the module is
    built.  Off, the module is the two F.cross_entropy calls.  The NSP term is
    F.cross_entropy either way: its logits are [B, 2], a few hundred bytes,
    and two launches of the fused kernels would buy nothing there.

    mlm_bias: the model's mlm_bias when mlm_logits come from
    model(..., add_mlm_bias=False).  With fused the kernels add it as they read
    the logits and return its gradient; without, it is added here.
    """

    def __init__(self, fused=None):
        super().__init__()
        if fused is None:
            fused = _fused_xent_default()
        self.fused = bool(fused)

    def forward(self, mlm_logits, nsp_logits, mlm_labels, nsp_labels,
                mlm_bias=None):
        if mlm_logits.dim() > 2:
            mlm_logits = mlm_logits.flatten(0, 1)
        mlm_labels = mlm_labels.flatten()
        if self.fused:
            mlm = softmax_cross_entropy(mlm_logits, mlm_labels,
                                        ignore_index=-100, bias=mlm_bias)
        else:
            if mlm_bias is not None:
                mlm_logits = mlm_logits + mlm_bias
            mlm = F.cross_entropy(mlm_logits, mlm_labels, ignore_index=-100)
        return mlm + F.cross_entropy(nsp_logits, nsp_labels)

    def extra_repr(self):
        return f"fused={self.fused}"


def bert_large(fused_ln=None, fused_gelu=None, fused_attn=None,
               fused_emb=None):
    return BertForPretraining(BERT_LARGE, fused_ln=fused_ln,
                              fused_gelu=fused_gelu, fused_attn=fused_attn,
                              fused_emb=fused_emb)


def bert_base(fused_ln=None, fused_gelu=None, fused_attn=None,
              fused_emb=None):
    return BertForPretraining(BERT_BASE, fused_ln=fused_ln,
                              fused_gelu=fused_gelu, fused_attn=fused_attn,
                              fused_emb=fused_emb)
