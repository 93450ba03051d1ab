"""Fused embedding + LayerNorm + dropout backed by the CDNA4 kernels in
csrc/emb_kernels.hip: the input block of a BERT model,
dropout(LayerNorm(tok[input_ids] + pos[0..S) + type[token_type_ids]), p), with
one gathered table row read and one row of the output dtype written per
token.

Forward is one kernel and saves only the row statistics.  Backward gathers the
sum again, writes the LayerNorm input gradient once as fp32 rows, and keeps
the position, type, weight and bias gradients in registers on the way (plus a
small fold); the token table's gradient is then a gather over the stably
sorted ids that writes every row of the table exactly once, zeros included:
no memset and no atomics, so identical inputs give identical bits.  The
dropout mask is the one of the fused LayerNorm kernels on a [B * S, H] tensor
(docs/api.md, "Fused embeddings"), with seed and offset from the device's
default torch generator, which every call with p > 0 advances by 4.

Input the kernels do not take (CPU tensors, ids that are not contiguous int64
[B, S], a row length that is not a multiple of 8 or above 4096, a type table
of more than 2 rows, non-contiguous or misaligned tables, tables that are
neither fp32 nor of the output dtype, p > 0 while a stream is capturing) goes
through the composite of F.embedding, F.layer_norm and F.dropout.
"""
import torch
import torch.nn.functional as F

from horovod_amd import _core
from horovod_amd.ops.fused_ln import (_DTYPES, MAX_H, _act_ok, _check_p,
                                      _next_philox)

MAX_TYPES = 2


def _composite(input_ids, token_type_ids, tok_weight, pos_weight, type_weight,
               ln_weight, ln_bias, p, eps, training, out_dtype):
    s = input_ids.shape[-1]
    pos = torch.arange(s, device=input_ids.device).unsqueeze(0)
    x = F.embedding(input_ids, tok_weight) + F.embedding(pos, pos_weight)
    if token_type_ids is not None:
        x = x + F.embedding(token_type_ids, type_weight)
    x = F.layer_norm(x, (x.shape[-1],), ln_weight, ln_bias, eps)
    x = F.dropout(x, p, training)
    return x if out_dtype is None else x.to(out_dtype)


def _ids_ok(ids, like):
    return (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
            and ids.device == like.device and ids.shape == like.shape)


def _dense_ok(w, ids, out_dtype):
    return w is None or (w.is_cuda and w.device == ids.device and
                         w.dtype in (torch.float32, out_dtype) and _act_ok(w))


def _eligible(input_ids, token_type_ids, tok_weight, pos_weight, type_weight,
              ln_weight, ln_bias, out_dtype, drop):
    """True when the native kernels take this call."""
    if out_dtype not in _DTYPES or input_ids.dim() != 2:
        return False
    if input_ids.numel() == 0 or not _ids_ok(input_ids, input_ids):
        return False
    if tok_weight.dim() != 2 or pos_weight.dim() != 2:
        return False
    H = tok_weight.shape[1]
    if H % 8 != 0 or not 8 <= H <= MAX_H or tok_weight.shape[0] < 1:
        return False
    # more positions than the table has rows: the composite raises
    if pos_weight.shape[1] != H or pos_weight.shape[0] < input_ids.shape[1]:
        return False
    if token_type_ids is not None and not (
            _ids_ok(token_type_ids, input_ids) and type_weight is not None and
            type_weight.dim() == 2 and type_weight.shape[1] == H and
            1 <= type_weight.shape[0] <= MAX_TYPES and
            _dense_ok(type_weight, input_ids, out_dtype)):
        return False
    for w in (ln_weight, ln_bias):
        if w is not None and w.shape != (H,):
            return False
    if not all(_dense_ok(w, input_ids, out_dtype)
               for w in (tok_weight, pos_weight, ln_weight, ln_bias)):
        return False
    # the generator's state cannot be read on the host while capturing
    if drop and torch.cuda.is_current_stream_capturing():
        return False
    return True


class _FusedEmbFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, input_ids, token_type_ids, tok_weight, pos_weight,
                type_weight, ln_weight, ln_bias, p, eps, out_dtype):
        seed, offset = _next_philox(input_ids.device) if p > 0.0 else (0, 0)
        if token_type_ids is None:
            type_weight = None
        y, mean, rstd = _core.fused_emb_forward(
            input_ids, token_type_ids, tok_weight, pos_weight, type_weight,
            ln_weight, ln_bias, p, eps, seed, offset, out_dtype)
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        ctx.bias_dtype = None if ln_bias is None else ln_bias.dtype
        ctx.save_for_backward(input_ids, token_type_ids, tok_weight,
                              pos_weight, type_weight, ln_weight, mean, rstd)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy):
        ids, types, tok, pos, typ, weight, mean, rstd = ctx.saved_tensors
        # the forward checked its inputs; the incoming gradient can still be
        # strided, or a contiguous view at an offset the 16-B loads cannot take
        dy = dy.contiguous()
        if dy.data_ptr() % 16 != 0:
            dy = dy.clone()
        grads = _core.fused_emb_backward(
            dy, ids, types, tok, pos, typ, weight, mean, rstd, ctx.p,
            ctx.seed, ctx.offset)
        dtypes = (tok.dtype, pos.dtype, None if typ is None else typ.dtype,
                  None if weight is None else weight.dtype, ctx.bias_dtype)
        out = [g.to(dt) if need and g is not None else None
               for g, dt, need in zip(grads, dtypes,
                                      ctx.needs_input_grad[2:7])]
        return (None, None, *out, None, None, None)


def embedding_layer_norm(input_ids, token_type_ids, tok_weight, pos_weight,
                         type_weight, ln_weight, ln_bias, p=0.0, eps=1e-5,
                         training=True, out_dtype=None):
    """dropout(LayerNorm(tok_weight[input_ids] + pos_weight[arange(S)] +
    type_weight[token_type_ids]), p) for input_ids [B, S]; token_type_ids
    (then no type row is added), ln_weight and ln_bias may be None.

    out_dtype None means the autocast dtype under autocast, else the token
    table's dtype.  With training False, or p == 0, nothing is dropped.
    """
    p = _check_p(p)
    drop = p if training else 0.0
    native_dtype = out_dtype
    if native_dtype is None:
        native_dtype = (torch.get_autocast_dtype("cuda")
                        if input_ids.is_cuda and
                        torch.is_autocast_enabled("cuda")
                        else tok_weight.dtype)
    if _eligible(input_ids, token_type_ids, tok_weight, pos_weight,
                 type_weight, ln_weight, ln_bias, native_dtype, drop > 0.0):
        return _FusedEmbFn.apply(input_ids, token_type_ids, tok_weight,
                                 pos_weight, type_weight, ln_weight, ln_bias,
                                 drop, eps, native_dtype)
    return _composite(input_ids, token_type_ids, tok_weight, pos_weight,
                      type_weight, ln_weight, ln_bias, p, eps, training,
                      out_dtype)
