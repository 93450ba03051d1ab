"""Fused dropout + add + LayerNorm on the GPU against an fp64 evaluation of
the definition in docs/api.md.

The reference runs on CPU copies of the already dtype-rounded inputs, with the
dropout mask taken from the host evaluation of the mask function
(fused_ln_keep_mask(..., "cpu")).  Forward: z, mean, rstd and y straight from
the definition.  Backward: fp64 from the z the forward returned (x where it
wrote none), with the statistics recomputed from it in fp64; measuring against
the unrounded z instead would charge the kernel for the rounding of a tensor
it has to store in the activations' dtype.

Tolerances are those of test_fused_bn_relu_matches_torch / test_gpu_syncbn.py,
|err| <= tol + tol * |ref|: fp32 everything 2e-4; fp16 / bf16 y, z, dz, dx
5e-2 and dgamma, dbeta 1e-2; mean and rstd 2e-4 in every dtype.

Shapes: rows {1, 3, 65, 257} (no multiple of a block's rows) x H {8, 64, 520,
768, 1024, 4096} (520 leaves a wave's last vector partly idle; 768 / 1024,
2048 and 4096 are the sizes at which the kernels spread a row over one, two
and four waves).  The grid test runs all 24 shapes with and without residual,
48 cases; dtype and p rotate over the cases by the rule in _grid() so that
every H, every row count, every dtype and every p appears both with and
without a residual (_grid() asserts it).
"""
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 65, 257]
HS = [8, 64, 520, 768, 1024, 4096]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PS = [0.0, 0.1, 0.5]
EPS = 1e-5
SEED, OFFSET = 0x0123_4567_89AB_CDEF, 12

ACT_TOL = {torch.float32: 2e-4, torch.bfloat16: 5e-2, torch.float16: 5e-2}
WGRAD_TOL = {torch.float32: 2e-4, torch.bfloat16: 1e-2, torch.float16: 1e-2}
STAT_TOL = 2e-4


def _grid():
    cases = []
    for i, (M, H) in enumerate(itertools.product(ROWS, HS)):
        r, c = divmod(i, len(HS))
        for has_res in (True, False):
            shift = 0 if has_res else 1
            dtype = DTYPES[(c + r + shift) % 3]
            p = PS[(c + 2 * r + 2 * shift) % 3]
            cases.append((M, H, dtype, p, has_res))
    # every H, row count, dtype and p, with and without a residual
    assert len(cases) == 48
    for has_res in (True, False):
        sub = [c for c in cases if c[4] == has_res]
        assert {c[0] for c in sub} == set(ROWS)
        assert {c[1] for c in sub} == set(HS)
        assert {c[2] for c in sub} == set(DTYPES)
        assert {c[3] for c in sub} == set(PS)
    return cases


def _id(case):
    M, H, dtype, p, has_res = case
    return f"{M}x{H}-{str(dtype)[6:]}-p{p}-{'res' if has_res else 'nores'}"


def _core():
    from horovod_amd import _core
    return _core


def _close(got, ref, tol, what):
    assert got is not None, what
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = tol + tol * ref.abs()
    ratio = float((err / bound).max())
    assert ratio <= 1.0, f"{what}: worst error / bound = {ratio:.3g}"
    return ratio


def _scale(p):
    t16 = min(max(round(p * 65536), 0), 65536)
    return 0.0 if t16 == 65536 else 65536.0 / (65536 - t16)


def _inputs(M, H, dtype, has_res, wdtype=torch.float32, bdtype=torch.float32,
            affine="both", seed=0):
    """dtype-rounded CPU tensors: x, residual, weight, bias, dy"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + H)
    x = torch.randn(M, H, generator=g).to(dtype)
    res = torch.randn(M, H, generator=g).to(dtype) if has_res else None
    w = (1 + 0.5 * torch.randn(H, generator=g)).to(wdtype)
    b = (0.5 * torch.randn(H, generator=g)).to(bdtype)
    dy = torch.randn(M, H, generator=g).to(dtype)
    if affine == "none":
        w = b = None
    elif affine == "weight":
        b = None
    return x, res, w, b, dy


def _ref_forward(x, res, w, b, p, seed, offset, eps=EPS):
    M, H = x.shape
    keep = _core().fused_ln_keep_mask(M, H, p, seed, offset, "cpu").double()
    z = keep * _scale(p) * x.double()
    if res is not None:
        z = res.double() + z
    mean = z.mean(-1)
    rstd = 1.0 / torch.sqrt(z.var(-1, unbiased=False) + eps)
    y = (z - mean[:, None]) * rstd[:, None]
    if w is not None:
        y = y * w.double()
    if b is not None:
        y = y + b.double()
    return y, z, mean, rstd, keep


def _ref_backward(dy, z_used, w, keep, p, eps=EPS):
    z = z_used.double()
    dy = dy.double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + eps)
    xhat = (z - mean) * rstd
    g = dy * w.double() if w is not None else dy
    dz = rstd * (g - g.mean(-1, keepdim=True) -
                 xhat * (g * xhat).mean(-1, keepdim=True))
    dx = dz * keep * _scale(p)
    return dz, dx, (dy * xhat).sum(0), dy.sum(0)


def _dev(t):
    return None if t is None else t.cuda()


def _check_native(M, H, dtype, p, has_res, seed=SEED, offset=OFFSET, **kw):
    """native forward + backward of one case against the fp64 reference"""
    core = _core()
    x, res, w, b, dy = _inputs(M, H, dtype, has_res, **kw)
    y, z, mean, rstd = core.fused_ln_forward(
        _dev(x), _dev(res), _dev(w), _dev(b), p, EPS, seed, offset, True)
    ry, rz, rmean, rrstd, keep = _ref_forward(x, res, w, b, p, seed, offset)
    tol = ACT_TOL[dtype]
    assert y.dtype == dtype and y.shape == x.shape
    _close(y, ry, tol, "y")
    assert mean.dtype == rstd.dtype == torch.float32
    _close(mean, rmean, STAT_TOL, "mean")
    _close(rstd, rrstd, STAT_TOL, "rstd")
    # z is written exactly when it is not x itself
    t16 = round(p * 65536)
    if has_res or t16 > 0:
        assert z is not None and z.dtype == dtype
        _close(z, rz, tol, "z")
        z_used = z
    else:
        assert z is None
        z_used = _dev(x)
    dz, dx, dgamma, dbeta = core.fused_ln_backward(
        _dev(dy), z_used, mean, rstd, _dev(w), p, seed, offset, True)
    rdz, rdx, rdg, rdb = _ref_backward(dy, z_used.cpu(), w, keep, p)
    _close(dz, rdz, tol, "dz")
    _close(dx, rdx, tol, "dx")
    if t16 == 0:
        assert dx.data_ptr() == dz.data_ptr()  # one tensor, written once
    assert dgamma.dtype == dbeta.dtype == torch.float32
    _close(dgamma, rdg, WGRAD_TOL[dtype], "dgamma")
    _close(dbeta, rdb, WGRAD_TOL[dtype], "dbeta")
    # without parameter gradients (another kernel instantiation and grid):
    # no dgamma / dbeta, and dz / dx held to the same reference
    dz2, dx2, dg2, db2 = core.fused_ln_backward(
        _dev(dy), z_used, mean, rstd, _dev(w), p, seed, offset, False)
    assert dg2 is None and db2 is None
    _close(dz2, rdz, tol, "dz without parameter gradients")
    _close(dx2, rdx, tol, "dx without parameter gradients")


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_matches_fp64_reference(case):
    _check_native(*case)


@pytest.mark.parametrize("H", [2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_two_waves_per_row(H, dtype):
    """1024 < H <= 2048 is the one kernel variant the issue's grid misses"""
    _check_native(65, H, dtype, 0.1, True)
    _check_native(3, 1032, dtype, 0.5, False)


@pytest.mark.parametrize("affine", ["both", "weight", "none"])
@pytest.mark.parametrize("param_t", [False, True], ids=["fp32", "T"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_affine_and_parameter_dtype(affine, param_t, dtype):
    pd = dtype if param_t else torch.float32
    _check_native(65, 768, dtype, 0.1, True, wdtype=pd, bdtype=pd,
                  affine=affine)


def test_mixed_parameter_dtypes():
    # weight and bias pick fp32 or T independently of each other
    _check_native(65, 768, torch.bfloat16, 0.1, True,
                  wdtype=torch.bfloat16, bdtype=torch.float32)
    _check_native(65, 768, torch.float16, 0.0, False,
                  wdtype=torch.float32, bdtype=torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_p_one_drops_everything(dtype):
    core = _core()
    _check_native(65, 768, dtype, 1.0, True)
    x, res, w, b, dy = _inputs(65, 768, dtype, True)
    y, z, mean, rstd = core.fused_ln_forward(
        x.cuda(), res.cuda(), w.cuda(), b.cuda(), 1.0, EPS, SEED, OFFSET,
        True)
    assert torch.equal(z.cpu(), res)
    ref = F.layer_norm(res.double(), (768,), w.double(), b.double(), EPS)
    _close(y, ref, ACT_TOL[dtype], "y = LN(residual)")
    dz, dx, _, _ = core.fused_ln_backward(
        dy.cuda(), z, mean, rstd, w.cuda(), 1.0, SEED, OFFSET, False)
    assert not bool(dx.any())
    assert dx.data_ptr() != dz.data_ptr()


def test_gpu_mask_equals_host_mask():
    core = _core()
    for p in (0.1, 0.5, 1.0, 0.0):
        host = core.fused_ln_keep_mask(65, 520, p, SEED, OFFSET, "cpu")
        dev = core.fused_ln_keep_mask(65, 520, p, SEED, OFFSET, "cuda")
        assert dev.is_cuda and dev.dtype == torch.uint8
        assert torch.equal(dev.cpu(), host)
    dev = core.fused_ln_keep_mask(3, 8, 0.5, 1, 2 ** 33, torch.device("cuda:0"))
    assert torch.equal(
        dev.cpu(), core.fused_ln_keep_mask(3, 8, 0.5, 1, 2 ** 33, "cpu"))


def _bounded(M, H, seed):
    """values in +-[1, 2]: kept elements move z and have a gradient"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (M, H), generator=g) * 2.0 - 1.0
    return sign * (1 + torch.rand(M, H, generator=g))


def test_implied_mask_of_a_real_forward():
    from horovod_amd.ops import FusedDropoutAddLayerNorm
    core = _core()
    M, H, p = 65, 520, 0.3
    mod = FusedDropoutAddLayerNorm(H, p=p).cuda().train()
    x = _bounded(M, H, 1).cuda().requires_grad_(True)
    res = torch.randn(M, H, generator=torch.Generator().manual_seed(2)).cuda()
    torch.manual_seed(77)
    gen = torch.cuda.default_generators[x.device.index]
    seed, offset = gen.initial_seed(), gen.get_offset()
    y = mod(x, res)
    assert gen.get_offset() == offset + 4
    host = core.fused_ln_keep_mask(M, H, p, seed, offset, "cpu").bool()
    z = y.grad_fn.saved_tensors[0]
    assert torch.equal((z != res).cpu(), host)
    # backward draws the same mask: dropped elements get no gradient.  The
    # weights below keep every dz away from an exact zero.
    w = torch.randn(M, H, generator=torch.Generator().manual_seed(3)).cuda()
    (y * w).sum().backward()
    assert torch.equal((x.grad != 0).cpu(), host)


def test_large_mean_uses_centred_variance():
    core = _core()
    M, H = 65, 1024
    g = torch.Generator().manual_seed(11)
    x = 100 + 0.5 * torch.randn(M, H, generator=g)
    res = 0.1 * torch.randn(M, H, generator=g)
    w = 1 + 0.5 * torch.randn(H, generator=g)
    b = 0.5 * torch.randn(H, generator=g)
    y, z, mean, rstd = core.fused_ln_forward(
        x.cuda(), res.cuda(), w.cuda(), b.cuda(), 0.0, EPS, 0, 0, True)
    ry, rz, rmean, rrstd, _ = _ref_forward(x, res, w, b, 0.0, 0, 0)
    _close(y, ry, 2e-4, "y")
    _close(z, rz, 2e-4, "z")
    _close(mean, rmean, 2e-4, "mean")
    _close(rstd, rrstd, 2e-4, "rstd")


@pytest.mark.parametrize("M,H,dtype", [(257, 1024, torch.bfloat16),
                                       (65, 4096, torch.float16),
                                       (257, 2048, torch.float32)])
def test_bitwise_reproducible(M, H, dtype):
    core = _core()
    x, res, w, b, dy = (t.cuda() for t in _inputs(M, H, dtype, True))
    outs = []
    for _ in range(2):
        y, z, mean, rstd = core.fused_ln_forward(x, res, w, b, 0.1, EPS, SEED,
                                                 OFFSET, True)
        outs.append([y, z, mean, rstd] + core.fused_ln_backward(
            dy, z, mean, rstd, w, 0.1, SEED, OFFSET, True))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_generator_governs_the_mask():
    from horovod_amd.ops import FusedDropoutAddLayerNorm
    mod = FusedDropoutAddLayerNorm(64, p=0.5).cuda().train()
    x = _bounded(65, 64, 5).cuda()
    res = torch.zeros_like(x)

    def mask_of_call():
        xx = x.clone().requires_grad_(True)
        y = mod(xx, res)
        return (y.grad_fn.saved_tensors[0] != 0).cpu()

    torch.manual_seed(1234)
    state = torch.cuda.get_rng_state()
    m1, m2 = mask_of_call(), mask_of_call()
    assert not torch.equal(m1, m2)
    assert 0.3 < m1.float().mean() < 0.7
    torch.cuda.set_rng_state(state)
    assert torch.equal(mask_of_call(), m1)
    assert torch.equal(mask_of_call(), m2)
    torch.manual_seed(1234)
    assert torch.equal(mask_of_call(), m1)
    torch.manual_seed(1235)
    assert not torch.equal(mask_of_call(), m1)
    # eval mode and p = 0 leave the generator alone
    before = torch.cuda.get_rng_state()
    mod.eval()
    mod(x, res)
    assert torch.equal(torch.cuda.get_rng_state(), before)


def _composite(mod, x, res, p, training):
    z = F.dropout(x, p, training)
    if res is not None:
        z = res + z
    return F.layer_norm(z, mod.normalized_shape, mod.weight, mod.bias,
                        mod.eps)


@pytest.mark.parametrize("kind", ["H12", "transposed", "2d-normalized"])
def test_fallbacks_compute_the_composite(kind):
    from horovod_amd.ops import FusedDropoutAddLayerNorm
    g = torch.Generator().manual_seed(9)
    if kind == "H12":
        shape, x = (12,), torch.randn(33, 12, generator=g).cuda()
    elif kind == "transposed":
        shape, x = (64,), torch.randn(64, 33, generator=g).cuda().t()
        assert not x.is_contiguous()
    else:
        shape, x = (8, 16), torch.randn(33, 8, 16, generator=g).cuda()
    res = torch.randn(x.shape, generator=g).cuda()
    mod = FusedDropoutAddLayerNorm(shape, p=0.3).cuda().train()
    with torch.no_grad():
        mod.weight.uniform_(0.5, 1.5)
        mod.bias.uniform_(-0.5, 0.5)
    x.requires_grad_(True)
    torch.manual_seed(5)
    out = mod(x, res)
    torch.manual_seed(5)
    ref = _composite(mod, x, res, 0.3, True)
    assert torch.equal(out, ref)
    gout, = torch.autograd.grad(out.sum(), x, retain_graph=True)
    gref, = torch.autograd.grad(ref.sum(), x)
    assert torch.equal(gout, gref)
    mod.eval()
    assert torch.equal(mod(x, res), _composite(mod, x, res, 0.3, False))


def test_native_entry_points_validate():
    core = _core()
    x = torch.randn(4, 64).cuda()
    w = torch.ones(64).cuda()

    def fwd(x_, res=None, w_=w, b_=None, p=0.0):
        return core.fused_ln_forward(x_, res, w_, b_, p, EPS, 0, 0, True)

    with pytest.raises(RuntimeError, match="GPU"):
        fwd(x, w_=w.cpu())
    with pytest.raises(RuntimeError):
        fwd(x, res=x.half())  # mixed dtypes
    with pytest.raises(RuntimeError):
        fwd(x.half(), w_=w.bfloat16())
    with pytest.raises(RuntimeError):
        fwd(torch.randn(4, 12).cuda(), w_=torch.ones(12).cuda())  # bad H
    with pytest.raises(RuntimeError):
        fwd(torch.randn(2, 4104).cuda(), w_=None)  # H above the maximum
    with pytest.raises(RuntimeError):
        fwd(torch.randn(4 * 64 + 1).cuda()[1:].view(4, 64))  # misaligned
    with pytest.raises(RuntimeError):
        fwd(torch.randn(64, 4).cuda().t())  # not contiguous
    with pytest.raises(RuntimeError):
        fwd(x, p=1.5)
    with pytest.raises(RuntimeError):
        fwd(x.double(), w_=None)
    y, z, mean, rstd = fwd(x)
    with pytest.raises(RuntimeError):
        core.fused_ln_backward(x, x, mean[:2], rstd, w, 0.0, 0, 0, True)
    with pytest.raises(RuntimeError):
        core.fused_ln_backward(x.half(), x, mean, rstd, w, 0.0, 0, 0, True)


def test_autocast_runs_in_the_dtype_it_is_handed():
    from horovod_amd.ops import FusedDropoutAddLayerNorm
    M, H, p = 65, 768, 0.1
    x, res, w, b, dy = _inputs(M, H, torch.bfloat16, True)
    mod = FusedDropoutAddLayerNorm(H, p=p).cuda().train()
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    xg = x.cuda().requires_grad_(True)
    rg = res.cuda().requires_grad_(True)
    torch.manual_seed(21)
    gen = torch.cuda.default_generators[xg.device.index]
    seed, offset = gen.initial_seed(), gen.get_offset()
    with torch.autocast("cuda", torch.bfloat16):
        y = mod(xg, rg)
    assert y.dtype == torch.bfloat16
    assert mod.weight.dtype == torch.float32
    ry, rz, _, _, keep = _ref_forward(x, res, w, b, p, seed, offset)
    _close(y, ry, 5e-2, "y")
    z = y.grad_fn.saved_tensors[0]
    assert z.dtype == torch.bfloat16
    y.backward(dy.cuda())
    rdz, rdx, rdg, rdb = _ref_backward(dy, z.cpu(), w, keep, p)
    assert xg.grad.dtype == rg.grad.dtype == torch.bfloat16
    _close(xg.grad, rdx, 5e-2, "dx")
    _close(rg.grad, rdz, 5e-2, "dresidual")
    assert mod.weight.grad.dtype == torch.float32
    _close(mod.weight.grad, rdg, 1e-2, "dgamma")
    _close(mod.bias.grad, rdb, 1e-2, "dbeta")
    # a residual of another dtype is cast to the branch's
    with torch.autocast("cuda", torch.bfloat16):
        y32 = mod.eval()(x.cuda(), res.cuda().float())
    assert y32.dtype == torch.bfloat16
    ry0 = _ref_forward(x, res, w, b, 0.0, 0, 0)[0]
    _close(y32, ry0, 5e-2, "y, fp32 residual")


def _tiny_bert(fused, dropout):
    from horovod_amd.models.bert import BertConfig, BertForPretraining
    cfg = BertConfig(vocab_size=100, hidden=64, layers=2, heads=4,
                     intermediate=128, max_seq=16, dropout=dropout)
    return BertForPretraining(cfg, fused_ln=fused)


def _bert_batch():
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 100, (4, 16), generator=g).cuda()
    types = torch.randint(0, 2, (4, 16), generator=g).cuda()
    labels = torch.randint(0, 100, (4, 16), generator=g).cuda()
    nsp = torch.randint(0, 2, (4,), generator=g).cuda()
    return ids, types, labels, nsp


def _bert_loss(model, batch):
    ids, types, labels, nsp = batch
    mlm, nsp_logits = model(ids, token_type_ids=types)
    return (F.cross_entropy(mlm.float().view(-1, 100), labels.view(-1)) +
            F.cross_entropy(nsp_logits.float(), nsp))


def test_misaligned_incoming_gradient():
    """a contiguous gradient at a storage offset that is not 16-byte aligned
    is copied, not handed to the kernels"""
    from horovod_amd.ops import FusedDropoutAddLayerNorm
    M, H = 33, 64
    x, res, w, b, dy = _inputs(M, H, torch.float32, True)
    mod = FusedDropoutAddLayerNorm(H, p=0.0).cuda().train()
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    xg = x.cuda().requires_grad_(True)
    y = mod(xg, res.cuda())
    assert type(y.grad_fn).__name__ == "_FusedLNFnBackward"
    buf = torch.zeros(M * H + 1, device="cuda")
    g = buf[1:].view(M, H)
    g.copy_(dy)
    assert g.is_contiguous() and g.data_ptr() % 16 != 0
    y.backward(g)
    z = (res.double() + x.double())
    rdz = _ref_backward(dy, z, w, torch.ones(M, H, dtype=torch.double), 0.0)[0]
    _close(xg.grad, rdz, 2e-4, "dx")


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16"])
def test_tiny_bert_every_layer_norm_is_fused(autocast):
    """the fused autograd node is behind the output of emb_norm, of every
    norm1 and norm2 and of the MLM head's LayerNorm: no site quietly takes
    the composite (nn.MultiheadAttention's transposed output once did that
    to norm1)"""
    from horovod_amd.ops import FusedDropoutAddLayerNorm, FusedLayerNorm
    torch.manual_seed(0)
    model = _tiny_bert(True, 0.1).cuda().train()
    seen = {}

    def hook(name):
        def fn(mod, args, out):
            seen[name] = (type(out.grad_fn).__name__, args[0].is_contiguous())
        return fn

    sites = [n for n, m in model.named_modules()
             if isinstance(m, (FusedLayerNorm, FusedDropoutAddLayerNorm))]
    assert sites == ["emb_norm",
                     "encoder.layers.0.norm1", "encoder.layers.0.norm2",
                     "encoder.layers.1.norm1", "encoder.layers.1.norm2",
                     "mlm_transform.2"]
    mods = dict(model.named_modules())
    for n in sites:
        mods[n].register_forward_hook(hook(n))
    ids, types, _, _ = _bert_batch()
    attn = torch.ones_like(ids)
    attn[1, 11:] = 0
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        model(ids, token_type_ids=types, attention_mask=attn)
    for n in sites:
        assert seen[n] == ("_FusedLNFnBackward", True), (n, seen[n])


def test_tiny_bert_step_matches_stock_fp32():
    torch.manual_seed(0)
    stock = _tiny_bert(False, 0.0).cuda().train()
    fused = _tiny_bert(True, 0.0).cuda().train()
    fused.load_state_dict(stock.state_dict(), strict=True)
    batch = _bert_batch()
    loss_s = _bert_loss(stock, batch)
    loss_f = _bert_loss(fused, batch)
    loss_s.backward()
    loss_f.backward()
    _close(loss_f, loss_s.detach().double().cpu(), 2e-4, "loss")
    grads_s = dict(stock.named_parameters())
    for name, pf in fused.named_parameters():
        assert pf.grad is not None, name
        _close(pf.grad, grads_s[name].grad.double().cpu(), 2e-4, name)


def test_tiny_bert_step_bf16_autocast_with_dropout():
    torch.manual_seed(0)
    fused = _tiny_bert(True, 0.1).cuda().train()
    with torch.autocast("cuda", torch.bfloat16):
        loss = _bert_loss(fused, _bert_batch())
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in fused.named_parameters():
        assert p.grad is not None, name
        assert bool(torch.isfinite(p.grad).all()), name
