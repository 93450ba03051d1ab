"""Fused bias + GELU + dropout on the GPU against an fp64 evaluation of
out = keep * scale * gelu(u + bias), du = dy * keep * scale * gelu'(u + bias),
dbias = du.sum(0), on CPU copies of the already dtype-rounded u, bias and dy
with the mask from fused_ln_keep_mask(..., "cpu").

|err| <= tol + tol * |ref|.  out, du: fp32 2e-4 (test_gpu_fused_ln.py's
figure), bf16 2^-8, fp16 2^-10: the kernel rounds once from fp32, so it is
within half an ulp plus its fp32 error of the reference.  Half an ulp is up to
2^-8 |ref| in bf16 and 2^-11 |ref| in fp16; for these inputs the fp64
reference rounded once reaches 0.78 (bf16) and 0.42 (fp16) of the bound, and
what is left is the absolute term, far above the fp32 error.  dbias: 2e-4 in
every dtype, it sums unrounded fp32 values.

Grid: rows {1, 3, 65, 257} x N {8, 64, 520, 1032, 3072, 4096}; 8 uses one
lane, 520 and 1032 leave one octet in a column tile of its own, 3072 and 4096
are the models' sizes.  Row chunks have at least 16 rows: 1 and 3 rows give a
single partial row (written straight into dbias), 65 and 257 rows five and
seventeen (folded).  dtype, p, the GELU form and the bias rotate by the rule
in _grid().
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_fused_ln import (_bert_batch, _bert_loss, _bounded,
                                     _close, _scale)

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 65, 257]
NS = [8, 64, 520, 1032, 3072, 4096]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PS = [0.0, 0.1, 0.5]
SEED, OFFSET = 0x0123_4567_89AB_CDEF, 12
TOL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def _grid():
    cases = []
    for i, (M, N) in enumerate(itertools.product(ROWS, NS)):
        r, c = divmod(i, len(NS))
        cases.append((M, N, DTYPES[(c + r) % 3], PS[(c + 2 * r) % 3],
                      (c + r) % 2 == 1, (c + r) // 2 % 2 == 0))
    # every dtype, p, form and bias choice with every N and every row count
    for key, vals in ((0, ROWS), (1, NS)):
        for v in vals:
            sub = [c for c in cases if c[key] == v]
            assert {c[2] for c in sub} == set(DTYPES)
            assert {c[3] for c in sub} == set(PS)
            assert {c[4] for c in sub} == {c[5] for c in sub} == {True, False}
    return cases


def _id(case):
    M, N, dtype, p, tanh, has_bias = case
    return (f"{M}x{N}-{str(dtype)[6:]}-p{p}-{'tanh' if tanh else 'erf'}-"
            f"{'bias' if has_bias else 'nobias'}")


def _core():
    from horovod_amd import _core
    return _core


def _inputs(M, N, dtype, has_bias, bdtype=torch.float32):
    g = torch.Generator().manual_seed(7 * M + N)
    u = torch.randn(M, N, generator=g).to(dtype)
    b = (0.5 * torch.randn(N, generator=g)).to(bdtype) if has_bias else None
    dy = torch.randn(M, N, generator=g).to(dtype)
    return u, b, dy


def _reference(u, b, dy, p, tanh, seed=SEED, offset=OFFSET):
    M, N = u.shape
    keep = _core().fused_ln_keep_mask(M, N, p, seed, offset, "cpu").double()
    v = u.double() if b is None else u.double() + b.double()
    v.requires_grad_(True)
    out = keep * _scale(p) * F.gelu(v, approximate="tanh" if tanh else "none")
    du, = torch.autograd.grad(out, v, dy.double())
    return out.detach(), du, du.sum(0)


def _dev(t):
    return None if t is None else t.cuda()


def _check_native(M, N, dtype, p, tanh, has_bias, **kw):
    core = _core()
    u, b, dy = _inputs(M, N, dtype, has_bias, **kw)
    r_out, r_du, r_db = _reference(u, b, dy, p, tanh)
    args = (_dev(b), p, SEED, OFFSET, tanh)
    out = core.fused_bias_gelu_forward(_dev(u), *args)
    assert out.dtype == dtype
    _close(out, r_out, TOL[dtype], "out")
    du, dbias = core.fused_bias_gelu_backward(_dev(dy), _dev(u), *args, True)
    assert du.dtype == dtype and dbias.dtype == torch.float32
    _close(du, r_du, TOL[dtype], "du")
    _close(dbias, r_db, 2e-4, "dbias")
    # without the bias gradient: another instantiation, the same du
    du2, none = core.fused_bias_gelu_backward(_dev(dy), _dev(u), *args, False)
    assert none is None and torch.equal(du2, du)
    return out, du


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_matches_fp64_reference(case):
    _check_native(*case)


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=lambda d: str(d)[6:])
def test_bias_in_the_activations_dtype(dtype):
    _check_native(65, 1032, dtype, 0.1, False, True, bdtype=dtype)


def test_p_one_drops_everything():
    out, du = _check_native(65, 520, torch.bfloat16, 1.0, True, True)
    assert not bool(out.any()) and not bool(du.any())


@pytest.mark.parametrize("M,N,dtype", [(257, 4096, torch.bfloat16),
                                       (65, 1032, torch.float32)])
def test_bitwise_reproducible(M, N, dtype):
    core = _core()
    u, b, dy = (t.cuda() for t in _inputs(M, N, dtype, True))
    runs = [[core.fused_bias_gelu_forward(u, b, 0.1, SEED, OFFSET, False)] +
            core.fused_bias_gelu_backward(dy, u, b, 0.1, SEED, OFFSET, False,
                                          True) for _ in range(2)]
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


def test_public_function_mask_and_generator():
    from horovod_amd.ops import bias_gelu_dropout
    M, N, p = 65, 520, 0.3
    # |x| in [1, 2]: gelu(x) and gelu'(x) are away from zero
    x = _bounded(M, N, 1).cuda().requires_grad_(True)
    torch.manual_seed(77)
    gen = torch.cuda.default_generators[x.device.index]
    seed, offset = gen.initial_seed(), gen.get_offset()
    out = bias_gelu_dropout(x, None, p)
    assert gen.get_offset() == offset + 4
    host = _core().fused_ln_keep_mask(M, N, p, seed, offset, "cpu").bool()
    assert torch.equal((out != 0).cpu(), host)
    out.sum().backward()
    assert torch.equal((x.grad != 0).cpu(), host)
    before = torch.cuda.get_rng_state()
    bias_gelu_dropout(x, None, p, training=False)
    bias_gelu_dropout(x, None, 0.0)
    assert torch.equal(torch.cuda.get_rng_state(), before)


def test_native_entry_points_validate():
    core = _core()
    x, b = torch.randn(4, 64).cuda(), torch.zeros(64).cuda()
    bad = [(x.cpu(), b), (x, b.cpu()), (x.half(), b.bfloat16()),
           (torch.randn(4, 12).cuda(), None),
           (torch.randn(4 * 64 + 1).cuda()[1:].view(4, 64), b),  # misaligned
           (torch.randn(64, 4).cuda().t(), None)]  # not contiguous
    for u_, b_ in bad:
        with pytest.raises(RuntimeError):
            core.fused_bias_gelu_forward(u_, b_, 0.0, 0, 0, False)
        with pytest.raises(RuntimeError):
            core.fused_bias_gelu_backward(u_, u_, b_, 0.0, 0, 0, False, True)
    with pytest.raises(RuntimeError):
        core.fused_bias_gelu_forward(x, b, 1.5, 0, 0, False)
    with pytest.raises(RuntimeError):
        core.fused_bias_gelu_backward(x.half(), x, b, 0.0, 0, 0, False, True)


def _tiny_bert(fused_gelu, dropout):
    from horovod_amd.models.bert import BertConfig, BertForPretraining
    cfg = BertConfig(vocab_size=100, hidden=64, layers=2, heads=4,
                     intermediate=128, max_seq=16, dropout=dropout)
    return BertForPretraining(cfg, fused_ln=fused_gelu, fused_gelu=fused_gelu)


def test_tiny_bert_step_matches_stock_fp32():
    torch.manual_seed(0)
    stock = _tiny_bert(False, 0.0).cuda().train()
    fused = _tiny_bert(True, 0.0).cuda().train()
    fused.load_state_dict(stock.state_dict(), strict=True)
    batch = _bert_batch()
    loss_s, loss_f = _bert_loss(stock, batch), _bert_loss(fused, batch)
    loss_s.backward()
    loss_f.backward()
    _close(loss_f, loss_s.detach().double().cpu(), 2e-4, "loss")
    grads_s = dict(stock.named_parameters())
    for name, pf in fused.named_parameters():
        _close(pf.grad, grads_s[name].grad.double().cpu(), 2e-4, name)


def test_tiny_bert_bf16_autocast_takes_the_fused_path():
    torch.manual_seed(0)
    fused = _tiny_bert(True, 0.1).cuda().train()
    sites = [fused.mlm_transform[0]] + [l.linear1 for l in fused.encoder.layers]
    seen = []
    for m in sites:
        m.register_forward_hook(
            lambda mod, args, out: seen.append(type(out.grad_fn).__name__))
    with torch.autocast("cuda", torch.bfloat16):
        loss = _bert_loss(fused, _bert_batch())
    loss.backward()
    assert seen == ["_FusedBiasGeluFnBackward"] * 3
    assert bool(torch.isfinite(loss))
    for name, p in fused.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
