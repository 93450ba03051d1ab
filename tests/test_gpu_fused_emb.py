"""Fused embedding + LayerNorm + dropout on the GPU against an fp64 CPU
evaluation of the definition in docs/api.md ("Fused embeddings").

The reference runs on CPU copies of the already dtype-rounded inputs, with the
dropout mask from the host evaluation fused_ln_keep_mask(B * S, H, ..., "cpu").
Bounds, |err| <= tol + tol * |ref|: y 2e-4 for fp32 and 5e-2 for 2-byte
outputs (ACT_TOL of test_gpu_fused_ln.py); mean, rstd and every gradient 2e-4
in every output dtype, because the backward reads no rounded intermediate
(fp32 tables, dy rounded before the reference sees it, fp32 dz) and adds at
most 9 * 33 = 297 fp32 terms per element.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, EPS = 11, 1e-5
ABSENT = 7  # the token id no case draws: its gradient row is exactly zero
SEED, OFFSET = 0x0123_4567_89AB_CDEF, 12
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PS = [0.0, 0.1, 0.5]
ACT_TOL = {torch.float32: 2e-4, torch.bfloat16: 5e-2, torch.float16: 5e-2}
TOL = 2e-4
# (B, S) x H with dtype, p and the type ids rotating so that each value occurs
CASES = [(B, S, H, DTYPES[(i + j) % 3], PS[(i + 2 * j) % 3], (i + j) % 2 == 0)
         for i, (B, S) in enumerate([(1, 1), (3, 5), (9, 33)])
         for j, H in enumerate([8, 520, 1024, 2048, 4096])]


def _close(got, ref, tol, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float(((got - ref).abs() / (tol + tol * ref.abs())).max())
    assert ratio <= 1.0, f"{what}: worst error / bound = {ratio:.3g}"


def _inputs(B, S, H, dtype, types):
    g = torch.Generator().manual_seed(7 * B + S + H)
    ids = torch.randint(0, V - 1, (B, S), generator=g)
    ids[ids >= ABSENT] += 1
    tt = torch.randint(0, 2, (B, S), generator=g) if types else None
    tok, pos, typ = (torch.randn(n, H, generator=g) for n in (V, S + 3, 2))
    w = 1 + 0.5 * torch.randn(H, generator=g)
    b = 0.5 * torch.randn(H, generator=g)
    dy = torch.randn(B, S, H, generator=g).to(dtype)
    return ids, tt, tok, pos, typ, w, b, dy


def _reference(ids, tt, tok, pos, typ, w, b, dy, p):
    """y, mean, rstd and the five gradients by autograd in fp64"""
    from horovod_amd import _core
    B, S = ids.shape
    H = tok.shape[1]
    tok, pos, typ, w, b = (t.double().requires_grad_(True)
                           for t in (tok, pos, typ, w, b))
    z = tok[ids] + pos[:S]
    if tt is not None:
        z = z + typ[tt]
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + EPS)
    t16 = round(p * 65536)
    keep = _core.fused_ln_keep_mask(B * S, H, p, SEED, OFFSET, "cpu")
    y = (keep.view(B, S, H).double() * (65536.0 / (65536 - t16)) *
         (w * (z - mean) * rstd + b))
    y.backward(dy.double())
    grads = [tok.grad, pos.grad, typ.grad if tt is not None else None,
             w.grad, b.grad]
    return y.detach(), mean.detach().flatten(), rstd.detach().flatten(), grads


def _native(ids, tt, tok, pos, typ, w, b, dy, p, dtype):
    from horovod_amd import _core
    dev = [None if t is None else t.cuda()
           for t in (ids, tt, tok, pos, typ, w, b, dy)]
    ids, tt, tok, pos, typ, w, b, dy = dev
    if tt is None:
        typ = None
    y, mean, rstd = _core.fused_emb_forward(
        ids, tt, tok, pos, typ, w, b, p, EPS, SEED, OFFSET, dtype)
    grads = _core.fused_emb_backward(dy, ids, tt, tok, pos, typ, w, mean,
                                     rstd, p, SEED, OFFSET)
    return y, mean, rstd, grads


@pytest.mark.parametrize(
    "case", CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{str(c[3])[6:]}-"
    f"p{c[4]}-{'types' if c[5] else 'notypes'}")
def test_matches_fp64_reference(case):
    B, S, H, dtype, p, types = case
    inputs = _inputs(B, S, H, dtype, types)
    y, mean, rstd, grads = _native(*inputs, p, dtype)
    ry, rmean, rrstd, rgrads = _reference(*inputs, p)
    assert y.dtype == dtype and mean.dtype == rstd.dtype == torch.float32
    _close(y, ry, ACT_TOL[dtype], "y")
    _close(mean, rmean, TOL, "mean")
    _close(rstd, rrstd, TOL, "rstd")
    names = ["dtok", "dpos", "dtype", "dgamma", "dbeta"]
    for name, got, ref in zip(names, grads, rgrads):
        if ref is None:
            assert got is None, name
            continue
        assert got.dtype == torch.float32, name
        _close(got, ref, TOL, name)
    assert not bool(grads[0][ABSENT].any())
    assert not bool(grads[1][S:].any())


def test_bitwise_reproducible():
    from horovod_amd.ops import embedding_layer_norm
    ids, tt, tok, pos, typ, w, b, dy = (
        t.cuda() for t in _inputs(9, 33, 1024, torch.bfloat16, True))
    params = [t.requires_grad_(True) for t in (tok, pos, typ, w, b)]
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        y = embedding_layer_norm(ids, tt, *params, p=0.5,
                                 out_dtype=torch.bfloat16)
        assert type(y.grad_fn).__name__ == "_FusedEmbFnBackward"
        runs.append([y, *torch.autograd.grad(y, params, dy)])
    assert not bool(runs[0][0].isnan().any())
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


def test_tiny_bert_matches_unfused_embeddings():
    from horovod_amd.models.bert import BertConfig, BertForPretraining
    cfg = BertConfig(vocab_size=100, hidden=64, layers=1, heads=4,
                     intermediate=128, max_seq=16, dropout=0.1)
    torch.manual_seed(0)
    plain = BertForPretraining(cfg, fused_ln=True, fused_emb=False)
    fused = BertForPretraining(cfg, fused_ln=True, fused_emb=True)
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict(), strict=True)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 100, (4, 16), generator=g).cuda()
    types = torch.randint(0, 2, (4, 16), generator=g).cuda()
    out = []
    for model in (plain, fused):
        model.cuda().eval()
        mlm, nsp = model(ids, token_type_ids=types)
        (mlm.square().mean() + nsp.square().mean()).backward()
        out.append([mlm] + [p.grad for p in (
            model.tok_emb.weight, model.pos_emb.weight, model.type_emb.weight,
            model.emb_norm.weight, model.emb_norm.bias)])
    for name, ref, got in zip(["logits", "dtok", "dpos", "dtype", "dgamma",
                               "dbeta"], *out):
        _close(got, ref.detach().double().cpu(), TOL, name)
