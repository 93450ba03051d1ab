"""Fused self-attention on the GPU against an fp64 evaluation of the
definition in docs/api.md ("Fused self-attention") on CPU copies of the
already dtype-rounded qkv and dout, with the dropout mask from
fused_ln_keep_mask(B * heads * S, S8, ..., "cpu")[:, :S] and the gradients from
torch.autograd.grad.

B = 2, heads = 2 (E = 128: batch and head strides both matter).  S: 1 (a
single key), 24 (under a tile, a multiple of 8 but not 16), 64 (one tile), 72
(a tile and an octet), 129 (two tiles and a key, S8 != S), 512 (the limit).
dtype, p and the mask form (none / lengths [S, max(1, S // 3)] / batch entry 1
fully padded) rotate by the rule in _grid().

out: |err| <= u |ref| + 3u (a @ |v|) + 1e-5, u = 2^-8 (bf16), 2^-11 (fp16):
one rounding of the output, one of each P entry and at most one in the
denominator, one more u for the fp32 arithmetic.
lse: |err| <= 1e-5 (1 + |ref|); -inf exactly for a sequence without keys.
dq, dk, dv: max|err| <= C u max|ref| per block, C = C_GRAD for all cases.  C is
twice the worst ratio max|err| / (u max|ref|) of the STOCK path (the
scaled_dot_product_attention core of FusedLNEncoderLayer._attention on views
of the same qkv, same dtype, on the GPU) against the same fp64 reference over
the grid's p = 0 cases, rounded up; both paths round P and dS once before the
second product but sum in different orders.  Measured on an MI355X, worst
ratio over dq / dk / dv and the p = 0 cases (the fully padded batch entry is
left out for the stock path, which gives NaN there):
  stock path  0.948 -> C = ceil(2 * 0.948) = 2
  fused path  0.948 (p = 0 cases), 1.337 (all cases)
In most cases the two paths give the same ratio to three digits: the largest
error is the rounding of the largest gradient elements to the dtype, which
both paths do once from nearly the same fp32 value.  A block whose reference
is identically zero (dq and dk at S = 1) is measured against max|ref| of the
whole dqkv instead; see _grad_ratios().
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_fused_ln import _scale

pytestmark = pytest.mark.gpu

B, HEADS, E = 2, 2, 128
SS = [1, 24, 64, 72, 129, 512]
DTYPES = [torch.bfloat16, torch.float16]
PS = [0.0, 0.1]
MASKS = ["none", "lengths", "padded"]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SEED, OFFSET = 0x0123_4567_89AB_CDEF, 12
C_GRAD = 2


def _grid():
    cases = [(S, DTYPES[(i + m) % 2], PS[(i + (m + 1) // 2) % 2], MASKS[m])
             for i, S in enumerate(SS) for m in range(3)]
    for S in SS:
        sub = [c for c in cases if c[0] == S]
        assert {c[1] for c in sub} == set(DTYPES)
        assert {c[2] for c in sub} == set(PS)
        assert {c[3] for c in sub} == set(MASKS)
    assert {c[3] for c in cases if c[2] == 0.0} == set(MASKS)
    return cases


def _id(case):
    S, dtype, p, mask = case
    return f"S{S}-{str(dtype)[6:]}-p{p}-{mask}"


def _core():
    from horovod_amd import _core
    return _core


def _inputs(S, dtype, mask):
    g = torch.Generator().manual_seed(11 * S + MASKS.index(mask))
    qkv = torch.randn(B, S, 3 * E, generator=g).to(dtype)
    dout = torch.randn(B, S, E, generator=g).to(dtype)
    lengths = {"none": None, "lengths": [S, max(1, S // 3)], "padded": [S, 0]}
    pad = None
    if lengths[mask] is not None:
        pad = torch.arange(S)[None, :] >= torch.tensor(lengths[mask])[:, None]
    return qkv, dout, pad


def _heads(t):
    return t.view(B, -1, HEADS, 64).transpose(1, 2)


def _reference(qkv, dout, pad, p):
    """-> out, lse, dqkv, a @ |v| (the out bound's middle term), all fp64"""
    S, S8 = qkv.shape[1], (qkv.shape[1] + 7) // 8 * 8
    x = qkv.double().requires_grad_(True)
    q, k, v = (_heads(t) for t in x.chunk(3, dim=-1))
    s = 0.125 * q @ k.transpose(-1, -2)
    ok = torch.ones(B, 1, 1, S, dtype=torch.bool) if pad is None \
        else ~pad[:, None, None, :]
    top = s.detach().masked_fill(~ok, -1e300).amax(-1, keepdim=True)
    e = torch.where(ok, s - top, 0.0).exp() * ok
    den = e.sum(-1, keepdim=True)
    prob = e / den.clamp_min(1e-300)  # zero rows for a sequence without keys
    lse = (den.log() + top).squeeze(-1).detach()  # -inf there
    keep = _core().fused_ln_keep_mask(B * HEADS * S, S8, p, SEED, OFFSET,
                                      "cpu")[:, :S].view(B, HEADS, S, S)
    a = keep.double() * _scale(p) * prob
    out = (a @ v).transpose(1, 2).reshape(B, S, E)
    dqkv, = torch.autograd.grad(out, x, dout.double())
    av = (a.detach() @ v.detach().abs()).transpose(1, 2).reshape(B, S, E)
    return out.detach(), lse, dqkv, av


def _out_ratio(out, r_out, av, u):
    err = (out.detach().double().cpu() - r_out).abs()
    return float((err / (u * r_out.abs() + 3 * u * av + 1e-5)).max())


def _grad_ratios(dqkv, r_dqkv, u, rows=slice(None)):
    got = dqkv.detach().double().cpu()
    # S = 1: dq and dk are identically zero in exact arithmetic (one key, p_ij
    # = 1, ds = 0), and no rounded dp - D is; such a block is measured against
    # max|ref| of the whole dqkv
    return [float((g[rows] - r[rows]).abs().max() /
                  (u * (r[rows].abs().max() or r_dqkv[rows].abs().max())))
            for g, r in zip(got.chunk(3, dim=-1), r_dqkv.chunk(3, dim=-1))]


def _sdpa(x, pad):
    """the stock core: SDPA on strided views of the packed tensor"""
    q, k, v = (_heads(t) for t in x.chunk(3, dim=-1))
    mask = None if pad is None else ~pad[:, None, None, :]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    return o.transpose(1, 2).reshape(B, -1, E)


def _dev(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_matches_fp64_reference(case):
    S, dtype, p, mask = case
    core, u = _core(), U[dtype]
    qkv, dout, pad = _inputs(S, dtype, mask)
    r_out, r_lse, r_dqkv, av = _reference(qkv, dout, pad, p)
    out, lse = core.fused_attention_forward(_dev(qkv), _dev(pad), HEADS, p,
                                            SEED, OFFSET)
    dqkv = core.fused_attention_backward(_dev(dout), _dev(qkv), out, lse,
                                         _dev(pad), HEADS, p, SEED, OFFSET)
    assert out.dtype == dqkv.dtype == dtype and lse.dtype == torch.float32
    assert out.shape == (B, S, E) and dqkv.shape == (B, S, 3 * E)
    ratios = _grad_ratios(dqkv, r_dqkv, u)
    print(f"{_id(case)}: out {_out_ratio(out, r_out, av, u):.3f} of the "
          f"bound, dq dk dv {ratios} u max|ref|")
    assert not bool(out.isnan().any()) and not bool(dqkv.isnan().any())
    assert _out_ratio(out, r_out, av, u) <= 1.0
    lse, finite = lse.double().cpu(), r_lse.isfinite()
    assert torch.equal(lse[~finite], r_lse[~finite])
    assert bool(((lse - r_lse).abs()[finite] <=
                 1e-5 * (1 + r_lse.abs()[finite])).all())
    assert max(ratios) <= C_GRAD
    if mask == "padded":
        assert not bool(out[1].any()) and not bool(dqkv[1].any())


def test_reproducible_and_p_one_drops_everything():
    core = _core()
    qkv, dout, pad = (_dev(t) for t in _inputs(129, torch.bfloat16, "lengths"))

    def run(p):
        out, lse = core.fused_attention_forward(qkv, pad, HEADS, p, SEED,
                                                OFFSET)
        return out, core.fused_attention_backward(dout, qkv, out, lse, pad,
                                                  HEADS, p, SEED, OFFSET)

    for a, b in zip(run(0.1), run(0.1)):
        assert torch.equal(a, b) and bool(a.any())
    for t in run(1.0):
        assert not bool(t.any())


def test_public_function_against_sdpa_and_generator():
    from horovod_amd.ops import self_attention
    S, dtype = 72, torch.bfloat16
    qkv, dout, pad = _inputs(S, dtype, "lengths")
    av = _reference(qkv, dout, pad, 0.0)[3]
    x = qkv.cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        out = self_attention(x, HEADS, pad.cuda(), 0.0)
        want = _sdpa(x, pad.cuda())
    assert type(out.grad_fn).__name__ == "_FusedSelfAttentionFnBackward"
    assert _out_ratio(out, want.detach().double().cpu(), av, U[dtype]) <= 1.0
    got, = torch.autograd.grad(out, x, dout.cuda())
    ref, = torch.autograd.grad(want, x, dout.cuda())
    assert max(_grad_ratios(got, ref.double().cpu(), U[dtype])) <= C_GRAD
    gen = torch.cuda.default_generators[x.device.index]
    offset = gen.get_offset()
    self_attention(x, HEADS, pad.cuda(), 0.1)
    assert gen.get_offset() == offset + 4
    self_attention(x, HEADS, pad.cuda(), 0.1, training=False)
    assert gen.get_offset() == offset + 4


def _behind(fn, name, depth=8):
    """True when a node called name is within depth steps behind fn"""
    if fn is None or depth == 0:
        return False
    return type(fn).__name__ == name or any(
        _behind(nxt, name, depth - 1) for nxt, _ in fn.next_functions)


def test_tiny_bert_takes_the_fused_attention():
    from horovod_amd.models.bert import BertConfig, BertForPretraining
    cfg = BertConfig(vocab_size=100, hidden=128, layers=2, heads=2,
                     intermediate=256, max_seq=16, dropout=0.0)
    torch.manual_seed(0)
    off = BertForPretraining(cfg, fused_ln=True, fused_attn=False).cuda().train()
    on = BertForPretraining(cfg, fused_ln=True, fused_attn=True).cuda().train()
    on.load_state_dict(off.state_dict(), strict=True)
    off.load_state_dict(on.state_dict(), strict=True)
    seen = []
    for layer in on.encoder.layers:
        layer.norm1.register_forward_pre_hook(
            lambda mod, args: seen.append(
                _behind(args[0].grad_fn, "_FusedSelfAttentionFnBackward")))
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 100, (4, 16), generator=g).cuda()
    types = torch.randint(0, 2, (4, 16), generator=g).cuda()
    attn = (torch.arange(16)[None, :] < torch.tensor([16, 5, 9, 1])[:, None])
    with torch.autocast("cuda", torch.bfloat16):
        mlm_on, nsp = on(ids, types, attn.long().cuda())
        mlm_off, _ = off(ids, types, attn.long().cuda())
    assert seen == [True, True]
    # one rounding of the logits, and 3u of their scale for what the two
    # attention cores leave different in bf16 upstream
    ref, u = mlm_off.detach().double(), U[torch.bfloat16]
    err = (mlm_on.detach().double() - ref).abs()
    assert bool((err <= u * ref.abs() + 3 * u * ref.abs().max()).all())
    (mlm_on.float().square().mean() + nsp.float().square().mean()).backward()
    for name, p in on.named_parameters():
        assert p.grad is not None and bool(p.grad.isfinite().all()), name
