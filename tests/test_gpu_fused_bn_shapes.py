"""Fused BatchNorm(+Add)+ReLU kernels over the shapes that reach each code
path of csrc/bn_kernels.hip, against BatchNorm training math in fp64.

The reference starts from the same, already-rounded inputs.  Its backward
takes the ReLU mask from the fused forward's own output (y_fused > 0), so no
near-zero element can flip the mask and a plain allclose applies to every
element.  Tolerances are the project's own from
test_fused_bn_relu_matches_torch: fp32 2e-4, bf16/fp16 5e-2 (rtol = atol),
dgamma/dbeta 1e-2, running mean 1e-4, running var 1e-3.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

EPS = 1e-5
MOMENTUM = 0.1

# (N, C, H, W): what it reaches
SHAPES = [
    (2, 8, 1, 1),       # C/8 = 1: fold across all 64 lanes; vectors < threads
    (1, 64, 17, 17),    # C/8 = 8 fold; 2312 vectors on 2 blocks: unrolled
                        # loop and a partial remainder loop both run
    (3, 256, 5, 5),     # C/8 = 32: last fold case
    (3, 512, 5, 5),     # C/8 = 64: first no-fold case
    (4, 24, 9, 7),      # C/8 not a power of two, grid rounded to its multiple
    (2, 40, 3, 3),      # same, C/8 = 5
    (2, 2048, 5, 5),    # wide C with few rows
    (1, 4096, 2, 2),    # the 32 KB LDS limit
    (8, 64, 56, 56),    # 4-deep loop runs more than once, grid cap active
]
DTYPES = [(torch.float32, 2e-4), (torch.bfloat16, 5e-2),
          (torch.float16, 5e-2)]


def _ids(v):
    if isinstance(v, tuple) and isinstance(v[0], int):
        return "x".join(map(str, v))
    if isinstance(v, tuple):
        return str(v[0]).replace("torch.", "")
    return str(v)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _close(got, exp, tol):
    return torch.allclose(got.double(), exp, rtol=tol, atol=tol)


def _err(got, exp):
    return float((got.double() - exp).abs().max())


def _make(shape, dtype, add, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n, c, h, w = shape

    def rnd(*s):
        return torch.randn(*s, device="cuda", generator=g)

    x = _cl(rnd(n, c, h, w).to(dtype))
    res = _cl(rnd(n, c, h, w).to(dtype)) if add else None
    dy = _cl(rnd(n, c, h, w).to(dtype))
    gamma = rnd(c) * 0.5 + 1.0
    beta = rnd(c) * 0.5
    return x, res, dy, gamma, beta


def _reference_forward(x, res, gamma, beta):
    xd = x.double()
    n = xd.numel() // xd.size(1)
    mean = xd.mean(dim=(0, 2, 3))
    var = xd.var(dim=(0, 2, 3), unbiased=False)
    invstd = (var + EPS).rsqrt()
    xhat = (xd - mean[None, :, None, None]) * invstd[None, :, None, None]
    z = xhat * gamma.double()[None, :, None, None] + \
        beta.double()[None, :, None, None]
    if res is not None:
        z = z + res.double()
    rm = MOMENTUM * mean
    rv = (1 - MOMENTUM) + MOMENTUM * var * (n / (n - 1) if n > 1 else 1.0)
    return z.clamp_min(0), xhat, invstd, rm, rv


def _reference_backward(xhat, invstd, gamma, dy, y_fused):
    n = xhat.numel() // xhat.size(1)
    g = torch.where(y_fused > 0, dy.double(), torch.zeros_like(xhat))
    sum_g = g.sum(dim=(0, 2, 3))
    sum_gx = (g * xhat).sum(dim=(0, 2, 3))
    dx = (gamma.double() * invstd)[None, :, None, None] * (
        g - (sum_g / n)[None, :, None, None] -
        xhat * (sum_gx / n)[None, :, None, None])
    return dx, g, sum_gx, sum_g


def _module(cls, c, gamma, beta):
    m = cls(c, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        m.weight.copy_(gamma)
        m.bias.copy_(beta)
    return m


@requires_gpu
@pytest.mark.parametrize("add", [False, True], ids=["relu", "add_relu"])
@pytest.mark.parametrize("dtype_tol", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fused_bn_shapes(shape, dtype_tol, add):
    from horovod_amd import _core
    from horovod_amd.ops import FusedBNAddReLU, FusedBNReLU
    dtype, tol = dtype_tol
    x, res, dy, gamma, beta = _make(shape, dtype, add)
    c = shape[1]
    m = _module(FusedBNAddReLU if add else FusedBNReLU, c, gamma, beta)
    xg = x.clone().requires_grad_(True)
    if add:
        rg = res.clone().requires_grad_(True)
        y = m(xg, rg)
    else:
        y = m(xg)
    assert y.dtype == dtype and y.shape == x.shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(dy)
    torch.cuda.synchronize()

    y_ref, xhat, invstd, rm, rv = _reference_forward(x, res, gamma, beta)
    dx_ref, g_ref, dgamma_ref, dbeta_ref = _reference_backward(
        xhat, invstd, gamma, dy, y.detach())
    print(f"{shape} {dtype} add={add}: y {_err(y, y_ref):.3g} "
          f"dx {_err(xg.grad, dx_ref):.3g} "
          f"dgamma {_err(m.weight.grad, dgamma_ref):.3g} "
          f"dbeta {_err(m.bias.grad, dbeta_ref):.3g} "
          f"rm {_err(m.running_mean, rm):.3g} "
          f"rv {_err(m.running_var, rv):.3g}")
    assert _close(y, y_ref, tol), _err(y, y_ref)
    assert torch.allclose(m.running_mean.double(), rm, atol=1e-4)
    assert torch.allclose(m.running_var.double(), rv, atol=1e-3)
    assert _close(xg.grad, dx_ref, tol), _err(xg.grad, dx_ref)
    assert _close(m.weight.grad, dgamma_ref, 1e-2)
    assert _close(m.bias.grad, dbeta_ref, 1e-2)
    if add:
        # the residual gradient is dy where the output is positive, else 0:
        # exact, and the backward apply pass reads it back instead of y + dy
        assert _close(rg.grad, g_ref, tol)
        assert torch.equal(
            rg.grad, torch.where(y.detach() > 0, dy, torch.zeros_like(dy)))
        # the same tensors through both backward variants: the one that
        # reads the stored g and the one that recomputes it from y and dy;
        # separate atomic reductions, so close but not bit-equal
        y2, mean, istd = _core.fused_bn_relu_forward(
            x, res, gamma, beta, torch.zeros(c, device="cuda"),
            torch.ones(c, device="cuda"), MOMENTUM, EPS)
        from_g = _core.fused_bn_relu_backward(x, y2, dy, mean, istd, gamma,
                                              True)
        from_y = _core.fused_bn_relu_backward(x, y2, dy, mean, istd, gamma,
                                              False)
        assert len(from_g) == 4 and len(from_y) == 3
        print(f"  dx from g vs from y, dy: "
              f"{_err(from_g[0], from_y[0].double()):.3g}")
        assert _close(from_g[0], from_y[0].double(), tol)
        assert _close(from_g[1], from_y[1].double(), 1e-2)
        assert _close(from_g[2], from_y[2].double(), 1e-2)
        assert torch.equal(
            from_g[3], torch.where(y2 > 0, dy, torch.zeros_like(dy)))


@requires_gpu
def test_unaligned_parameters_match_aligned():
    """weight, bias and running stats that are views at an odd element offset
    into a flat buffer (4 bytes past a 16-byte boundary) give the results of
    aligned ones."""
    from horovod_amd.ops import FusedBNReLU
    shape, dtype, tol = (4, 24, 9, 7), torch.float32, 2e-4
    x, _, dy, gamma, beta = _make(shape, dtype, False, seed=1)
    c = shape[1]
    aligned = _module(FusedBNReLU, c, gamma, beta)
    odd = FusedBNReLU(c, eps=EPS, momentum=MOMENTUM).cuda().train()
    flat = torch.zeros(4 * c + 4, device="cuda")
    flat[1:1 + c] = gamma
    flat[1 + c:1 + 2 * c] = beta
    flat[1 + 3 * c:1 + 4 * c] = 1.0
    odd.weight = torch.nn.Parameter(flat[1:1 + c])
    odd.bias = torch.nn.Parameter(flat[1 + c:1 + 2 * c])
    odd.running_mean = flat[1 + 2 * c:1 + 3 * c]
    odd.running_var = flat[1 + 3 * c:1 + 4 * c]
    for t in (odd.weight, odd.bias, odd.running_mean, odd.running_var):
        assert t.data_ptr() % 16 != 0
    outs = []
    for m in (aligned, odd):
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.backward(dy)
        outs.append((y.detach(), xg.grad, m.weight.grad, m.bias.grad,
                     m.running_mean, m.running_var))
    torch.cuda.synchronize()
    names = ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")
    tols = (tol, tol, 1e-2, 1e-2, 1e-4, 1e-3)
    for name, a, o, t in zip(names, outs[0], outs[1], tols):
        print(name, _err(o, a.double()))
        assert _close(o, a.double(), t), name
    # and the unaligned module is right on its own: fp64 reference
    y_ref, xhat, invstd, rm, rv = _reference_forward(x, None, gamma, beta)
    dx_ref, _, dgamma_ref, dbeta_ref = _reference_backward(
        xhat, invstd, gamma, dy, outs[1][0])
    assert _close(outs[1][0], y_ref, tol)
    assert _close(outs[1][1], dx_ref, tol)
    assert _close(outs[1][2], dgamma_ref, 1e-2)
    assert _close(outs[1][3], dbeta_ref, 1e-2)
    assert torch.allclose(outs[1][4].double(), rm, atol=1e-4)
    assert torch.allclose(outs[1][5].double(), rv, atol=1e-3)


@requires_gpu
def test_resnet_stem_fused_keeps_state_dict():
    """With fused_bn the stem's bn1 is a FusedBNReLU; parameter names and
    shapes stay, and a train-mode step runs on both variants."""
    from horovod_amd.models import resnet50
    from horovod_amd.ops import FusedBNReLU
    losses = []
    sds = []
    for fused in (True, False):
        torch.manual_seed(5)
        model = resnet50(fused_bn=fused).cuda().to(
            memory_format=torch.channels_last).train()
        assert isinstance(model.bn1, FusedBNReLU) == fused
        sds.append({k: tuple(v.shape) for k, v in model.state_dict().items()})
        g = torch.Generator(device="cuda")
        g.manual_seed(6)
        data = _cl(torch.randn(2, 3, 64, 64, device="cuda", generator=g))
        target = torch.tensor([1, 7], device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(model(data), target)
        loss.backward()
        assert all(p.grad is not None for p in model.parameters())
        losses.append(float(loss))
    assert sds[0] == sds[1]
    assert list(sds[0]) == list(sds[1])
    assert all(torch.isfinite(torch.tensor(losses))), losses
