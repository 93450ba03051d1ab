"""The persistent bank workspace of the fused BatchNorm(+Add)+ReLU path and
the backward that recomputes the ReLU mask from x instead of reading y.

Reference math, helpers and tolerances are those of
test_gpu_fused_bn_shapes.py (BatchNorm training math in fp64 from the same,
already-rounded inputs; backward mask taken from the fused forward's own y):
fp32 2e-4, bf16/fp16 5e-2 (rtol = atol), dgamma/dbeta 1e-2, running mean
1e-4, running var 1e-3.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
MOMENTUM = 0.1

# One process, one stream, in this order: a bank word that a wide layer left
# non-zero would be added into the sums of the narrower one that follows.
ORDER = [(2, 2048, 5, 5), (1, 64, 17, 17), (4, 24, 9, 7), (1, 4096, 2, 2),
         (2, 8, 1, 1), (2, 2048, 5, 5)]
DTYPES = [(torch.bfloat16, 5e-2), (torch.float32, 2e-4)]


def _ids(v):
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


# inputs and the fp64 forward reference of layer i of ORDER, made once per
# dtype and left unchanged; the backward reference needs the run's own y
_CASES = {}


def _case(i, dtype):
    key = (i, dtype)
    if key not in _CASES:
        add = i % 2 == 1  # FusedBNReLU and FusedBNAddReLU alternate
        x, res, dy, gamma, beta = _make(ORDER[i], dtype, add, seed=10 + i)
        _CASES[key] = (add, x, res, dy, gamma, beta,
                       _reference_forward(x, res, gamma, beta))
    return _CASES[key]


class _Layer:
    def __init__(self, i, dtype):
        from horovod_amd.ops import FusedBNAddReLU, FusedBNReLU
        self.i = i
        self.add, self.x, self.res, self.dy, gamma, beta, _ = _case(i, dtype)
        self.m = _module(FusedBNAddReLU if self.add else FusedBNReLU,
                         ORDER[i][1], gamma, beta)

    def forward(self):
        self.xg = self.x.clone().requires_grad_(True)
        if self.add:
            self.rg = self.res.clone().requires_grad_(True)
            self.y = self.m(self.xg, self.rg)
        else:
            self.y = self.m(self.xg)

    def backward(self):
        self.y.backward(self.dy)

    def check(self, dtype, tol):
        _, x, res, dy, gamma, beta, fwd = _case(self.i, dtype)
        y_ref, xhat, invstd, rm, rv = fwd
        y = self.y.detach()
        dx_ref, g_ref, dgamma_ref, dbeta_ref = _reference_backward(
            xhat, invstd, gamma, dy, y)
        m = self.m
        print(f"#{self.i} {ORDER[self.i]} {dtype} add={self.add}: "
              f"y {_err(y, y_ref):.3g} dx {_err(self.xg.grad, dx_ref):.3g} "
              f"dgamma {_err(m.weight.grad, dgamma_ref):.3g} "
              f"dbeta {_err(m.bias.grad, dbeta_ref):.3g} "
              f"rm {_err(m.running_mean, rm):.3g} "
              f"rv {_err(m.running_var, rv):.3g}")
        where = f"layer {self.i} {ORDER[self.i]}"
        assert _close(y, y_ref, tol), where
        assert torch.allclose(m.running_mean.double(), rm, atol=1e-4), where
        assert torch.allclose(m.running_var.double(), rv, atol=1e-3), where
        assert _close(self.xg.grad, dx_ref, tol), where
        assert _close(m.weight.grad, dgamma_ref, 1e-2), where
        assert _close(m.bias.grad, dbeta_ref, 1e-2), where
        if self.add:
            assert torch.equal(
                self.rg.grad, torch.where(y > 0, dy, torch.zeros_like(dy)))


def _run_order(dtype, pairwise):
    layers = [_Layer(i, dtype) for i in range(len(ORDER))]
    if pairwise:
        # two forwards before their two backwards: a layer's results must
        # survive another layer's use of the banks
        for a, b in zip(layers[0::2], layers[1::2]):
            a.forward()
            b.forward()
            b.backward()
            a.backward()
    else:
        for layer in layers:
            layer.forward()
            layer.backward()
    return layers


@requires_gpu
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["back_to_back", "two_forwards_first"])
@pytest.mark.parametrize("dtype_tol", DTYPES, ids=_ids)
def test_banks_clean_between_layers(dtype_tol, pairwise):
    dtype, tol = dtype_tol
    layers = _run_order(dtype, pairwise)
    torch.cuda.synchronize()
    for layer in layers:
        layer.check(dtype, tol)


@requires_gpu
def test_banks_clean_on_side_stream():
    """The same order on a non-default stream, which gets a workspace of its
    own, and then once more on the default stream."""
    dtype, tol = DTYPES[0]
    for i in range(len(ORDER)):
        _case(i, dtype)  # inputs are made on the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layers = _run_order(dtype, False)
    side.synchronize()
    for layer in layers:
        layer.check(dtype, tol)
    layers = _run_order(dtype, True)
    torch.cuda.synchronize()
    for layer in layers:
        layer.check(dtype, tol)


EDGE_SHAPE = (4, 64, 9, 9)


@requires_gpu
@pytest.mark.parametrize(
    "dtype_tol", DTYPES + [(torch.float16, 5e-2)], ids=_ids)
def test_mask_from_x_is_exact_on_the_edge(dtype_tol):
    """14 % of the elements get a pre-activation within one fp32 ulp of zero
    (positive, zero and negative ones, per channel); the backward that
    recomputes the mask from x must see exactly the forward's y > 0.

    x is integer-valued in [-3, 3], so sums, mean and invstd are the same in
    every run; dy is integer-valued and never 0, so sum(g) is exact in fp32
    in any order and dbeta can be compared bit for bit."""
    from horovod_amd import _core
    dtype, tol = dtype_tol
    n, c, h, w = EDGE_SHAPE
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = _cl(torch.randint(-3, 4, EDGE_SHAPE, device="cuda",
                          generator=g).to(dtype))
    mag = torch.randint(1, 4, EDGE_SHAPE, device="cuda", generator=g)
    sign = torch.randint(0, 2, EDGE_SHAPE, device="cuda", generator=g) * 2 - 1
    dy = _cl((mag * sign).to(dtype))
    gamma = torch.randn(c, device="cuda", generator=g) * 0.5 + 1.0

    def stats():
        return torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")

    _, mean, invstd = _core.fused_bn_relu_forward(
        x, None, gamma, torch.zeros(c, device="cuda"), *stats(), MOMENTUM,
        EPS)
    ch = torch.arange(c, device="cuda")
    v = (ch % 7 - 3).float()
    p = ((v - mean) * invstd) * gamma  # fp32, one rounding per step
    beta = -p
    up = torch.nextafter(beta, torch.full_like(beta, float("inf")))
    down = torch.nextafter(beta, torch.full_like(beta, float("-inf")))
    beta = torch.where(ch % 3 == 1, up, torch.where(ch % 3 == 2, down, beta))

    y, mean2, invstd2 = _core.fused_bn_relu_forward(
        x, None, gamma, beta, *stats(), MOMENTUM, EPS)
    assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd)
    edge = x.float() == v[None, :, None, None]
    n_edge = int(edge.sum())
    pos = int((y[edge] > 0).sum())
    zero = int((y[edge] == 0).sum())
    print(f"{dtype}: {n_edge} edge elements of {x.numel()}, "
          f"y > 0 on {pos}, y == 0 on {zero}")
    assert pos > 0 and zero > 0 and pos + zero == n_edge, \
        "the edge elements do not exercise both sides of the mask"

    from_x = _core.fused_bn_relu_backward(x, y, dy, mean2, invstd2, gamma,
                                          False, beta)
    no_y = _core.fused_bn_relu_backward(x, None, dy, mean2, invstd2, gamma,
                                        False, beta)
    from_y = _core.fused_bn_relu_backward(x, y, dy, mean2, invstd2, gamma,
                                          False)
    torch.cuda.synchronize()
    assert len(from_x) == 3 and len(no_y) == 3 and len(from_y) == 3

    _, xhat, invstd_ref, _, _ = _reference_forward(x, None, gamma, beta)
    dx_ref, _, dgamma_ref, dbeta_ref = _reference_backward(
        xhat, invstd_ref, gamma, dy, y)
    dbeta_exact = dbeta_ref.float()
    print(f"  dbeta max |from x - exact| "
          f"{_err(from_x[2], dbeta_exact.double()):.3g}, "
          f"dx {_err(from_x[0], dx_ref):.3g}, "
          f"dgamma {_err(from_x[1], dgamma_ref):.3g}")
    assert torch.equal(from_x[2], dbeta_exact)
    assert torch.equal(no_y[2], dbeta_exact)
    assert torch.equal(from_y[2], from_x[2])
    for outs in (from_x, no_y):
        assert _close(outs[0], dx_ref, tol), _err(outs[0], dx_ref)
        assert _close(outs[1], dgamma_ref, 1e-2)


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import test_gpu_fused_bn_workspace as t
from horovod_amd import _core
assert not _core.fused_bn_lean_path()
out = []
for dtype, _ in t.DTYPES:
    for layer in t._run_order(dtype, False):
        m = layer.m
        out.append([v.detach().cpu() for v in (
            layer.y, layer.xg.grad, m.weight.grad, m.bias.grad,
            m.running_mean, m.running_var)])
torch.cuda.synchronize()
torch.save(out, sys.argv[2])
"""


@requires_gpu
def test_switch_selects_the_earlier_path(tmp_path):
    """HOROVOD_FUSED_BN_WORKSPACE=0 in a child process: per-call banks and
    the y-reading backward give the default path's results."""
    from horovod_amd import _core
    assert _core.fused_bn_lean_path()
    dump = tmp_path / "switch_off.pt"
    env = dict(os.environ, HOROVOD_FUSED_BN_WORKSPACE="0")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"),
         str(dump)],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    off = torch.load(dump)
    k = 0
    names = ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")
    for dtype, tol in DTYPES:
        layers = _run_order(dtype, False)
        torch.cuda.synchronize()
        for layer in layers:
            m = layer.m
            on = (layer.y, layer.xg.grad, m.weight.grad, m.bias.grad,
                  m.running_mean, m.running_var)
            tols = (tol, tol, 1e-2, 1e-2, 1e-4, 1e-3)
            for name, a, b, t in zip(names, on, off[k], tols):
                assert _close(a.detach().cpu(), b.double(), t), \
                    (name, layer.i, dtype, _err(a.detach().cpu(), b.double()))
            k += 1


@requires_gpu
def test_backward_signatures():
    """8-argument forward -> 3 results; 7-argument backward -> 3 or 4, and it
    reads y: with a y of zeros every gradient is zero."""
    from horovod_amd import _core
    shape, dtype = (4, 24, 9, 7), torch.float32
    x, res, dy, gamma, beta = _make(shape, dtype, True, seed=2)
    c = shape[1]
    outs = _core.fused_bn_relu_forward(
        x, res, gamma, beta, torch.zeros(c, device="cuda"),
        torch.ones(c, device="cuda"), MOMENTUM, EPS)
    assert len(outs) == 3
    y, mean, invstd = outs
    assert mean.data_ptr() % 16 == 0 and invstd.data_ptr() % 16 == 0
    assert len(_core.fused_bn_relu_backward(x, y, dy, mean, invstd, gamma,
                                            True)) == 4
    zeros = _core.fused_bn_relu_backward(x, torch.zeros_like(y), dy, mean,
                                         invstd, gamma, False)
    assert len(zeros) == 3
    assert all(float(t.abs().max()) == 0.0 for t in zeros)
    # beta with a residual gradient wanted: the mask still comes from y
    with_beta = _core.fused_bn_relu_backward(x, torch.zeros_like(y), dy, mean,
                                             invstd, gamma, True, beta)
    assert len(with_beta) == 4
    assert all(float(t.abs().max()) == 0.0 for t in with_beta)
    with pytest.raises(RuntimeError):
        _core.fused_bn_relu_backward(x, None, dy, mean, invstd, gamma, False)
