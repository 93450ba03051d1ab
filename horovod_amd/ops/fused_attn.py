"""Fused multi-head self-attention backed by the CDNA4 matrix-instruction
kernels in csrc/attn_kernels.hip: softmax(q k^T / 8) v with key padding and
dropout, straight on the packed in_proj output qkv [B, S, 3E] (q | k | v as
nn.MultiheadAttention lays them out, head h in columns 64h .. 64h + 63 of
each).  The output is [B, S, E] with the heads merged, and the backward
writes one packed [B, S, 3E] gradient: no head split, no head merge and no
three-way concatenation by autograd.

Nothing is saved beyond qkv, the output, the [B, heads, S] fp32 log-sum-exp
and the mask argument; the probabilities are recomputed in the backward.  The
dropout mask is the one of the fused LayerNorm kernels (docs/api.md, "Fused
self-attention" has the indexing): a function of (seed, offset, element
index), with seed and offset from the device's default torch generator, which
every call with p > 0 advances by 4.

A sequence whose keys are all padding gets a zero output and zero gradients
(the stock softmax gives NaN there).

Input the kernels do not take (CPU tensors, fp32, a head dimension other than
64, S > 512, non-contiguous or misaligned tensors, p > 0 while a stream is
capturing) goes through the composite: F.scaled_dot_product_attention on
strided views of qkv.
"""
import torch
import torch.nn.functional as F

from horovod_amd import _core
from horovod_amd.ops.fused_ln import _act_ok, _check_p, _next_philox

HEAD_DIM = 64
MAX_S = 512
_DTYPES = (torch.float16, torch.bfloat16)


def _composite(qkv, num_heads, key_padding_mask, p, training):
    b, s, e3 = qkv.shape
    e = e3 // 3
    q, k, v = (t.view(b, s, num_heads, e // num_heads).transpose(1, 2)
               for t in qkv.chunk(3, dim=-1))
    mask = None
    if key_padding_mask is not None:
        # True marks padding there, "may attend" here
        mask = ~key_padding_mask.bool()[:, None, None, :]
    o = F.scaled_dot_product_attention(
        q, k, v, attn_mask=mask, dropout_p=p if training else 0.0)
    return o.transpose(1, 2).reshape(b, s, e)


def _eligible(qkv, num_heads, key_padding_mask, drop):
    """True when the native kernels take this call."""
    if not (qkv.is_cuda and qkv.dtype in _DTYPES and _act_ok(qkv)):
        return False
    b, s, e3 = qkv.shape
    if e3 != 3 * HEAD_DIM * num_heads or not 1 <= s <= MAX_S or b < 1:
        return False
    m = key_padding_mask
    if m is not None and not (m.is_cuda and m.device == qkv.device and
                              m.dtype == torch.bool and m.shape == (b, s) and
                              m.is_contiguous()):
        return False
    # the generator's state cannot be read on the host while capturing
    if drop and torch.cuda.is_current_stream_capturing():
        return False
    return True


class _FusedSelfAttentionFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, qkv, key_padding_mask, heads, p):
        seed, offset = _next_philox(qkv.device) if p > 0.0 else (0, 0)
        out, lse = _core.fused_attention_forward(qkv, key_padding_mask, heads,
                                                 p, seed, offset)
        ctx.heads, ctx.p, ctx.seed, ctx.offset = heads, p, seed, offset
        ctx.save_for_backward(qkv, out, lse, key_padding_mask)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        qkv, out, lse, mask = ctx.saved_tensors
        # the forward checked its inputs; the incoming gradient can still be
        # strided, or a contiguous view at an offset the 16-B loads cannot take
        dout = dout.contiguous()
        if dout.data_ptr() % 16 != 0:
            dout = dout.clone()
        dqkv = _core.fused_attention_backward(
            dout, qkv, out, lse, mask, ctx.heads, ctx.p, ctx.seed,
            ctx.offset)
        return dqkv, None, None, None


def self_attention(qkv, num_heads, key_padding_mask=None, p=0.0,
                   training=True):
    """Multi-head self-attention on a packed qkv [B, S, 3E]; -> [B, S, E].
    key_padding_mask: [B, S] bool, True = padding key.  With training False,
    or p == 0, nothing is dropped."""
    p = _check_p(p)
    if qkv.dim() != 3 or qkv.shape[-1] % (3 * num_heads) != 0:
        raise ValueError(
            f"qkv has to be [B, S, 3 * E] with E a multiple of num_heads = "
            f"{num_heads}, but got {tuple(qkv.shape)}")
    drop = p if training else 0.0
    if _eligible(qkv, num_heads, key_padding_mask, drop > 0.0):
        return _FusedSelfAttentionFn.apply(qkv, key_padding_mask, num_heads,
                                           drop)
    return _composite(qkv, num_heads, key_padding_mask, p, training)
