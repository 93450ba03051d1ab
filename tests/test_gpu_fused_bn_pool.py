"""The stem's fused BatchNorm+ReLU+MaxPool(3, 2, 1) kernels
(csrc/bn_pool_kernels.hip) against the two-op path they replace.

Exactness cases call single passes with caller-supplied statistics
(_core.fused_bn_pool_pass) and compare bit for bit with the existing pass
(_core.fused_bn_pass) followed or preceded by ATen's max-pool.  The existing
backward-apply probe pass takes mean / invstd as its sum_g / sum_gx, so the
new pass is given the same two arrays as sums.

End-to-end cases compare the module with BatchNorm training math in fp64,
with the tolerances of test_gpu_fused_bn_shapes.py: fp32 2e-4, bf16/fp16 5e-2
(rtol = atol), dgamma/dbeta 1e-2, running mean 1e-4, running var 1e-3.  The
forward is compared with the plain fp64 composite batch_norm -> relu ->
max_pool2d.  As in that file, the backward reference takes its routing from
the fused forward itself (the arg-max codes it saved, and pooled > 0 as the
ReLU mask of the arg-max element): values that tie after rounding to bf16 pick
a different element than their fp64 originals would, which moves a whole
gradient to a neighbour and is no error.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
MOMENTUM = 0.1

# (N, C, H, W): what it covers
SHAPES = [
    (2, 8, 7, 7),        # odd size, every border clipped
    (2, 64, 8, 8),       # even size: the last window ends on the last pixel
    (1, 72, 9, 10),      # C not a power of two, H != W
    (2, 16, 1, 1),       # windows that are mostly padding
    (2, 16, 2, 3),
    (1, 64, 112, 112),   # the stem's spatial size
]
TOL = {torch.float32: 2e-4, torch.bfloat16: 5e-2, torch.float16: 5e-2}
# bf16 on every shape, fp16 and fp32 on the first three
CASES = [(s, torch.bfloat16) for s in SHAPES] + \
        [(s, d) for d in (torch.float16, torch.float32) for s in SHAPES[:3]]


def _id(case):
    shape, dtype = case
    return "x".join(map(str, shape)) + "-" + str(dtype).replace("torch.", "")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _close(got, exp, tol):
    return torch.allclose(got.double(), exp, rtol=tol, atol=tol)


def _err(got, exp):
    return float((got.double() - exp).abs().max())


def _pooled_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _flat_index(codes, h, w):
    """Window codes kh * 3 + kw -> ATen's flat index ih * W + iw."""
    oh, ow = codes.shape[2:]
    c = codes.long()
    ih = 2 * torch.arange(oh, device=codes.device)[:, None] - 1 + c // 3
    iw = 2 * torch.arange(ow, device=codes.device)[None, :] - 1 + c % 3
    assert int(ih.min()) >= 0 and int(ih.max()) < h
    assert int(iw.min()) >= 0 and int(iw.max()) < w
    return ih * w + iw


def _stats(c, seed):
    """Caller-supplied mean, invstd, gamma, beta (fp32 [C])."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def rnd():
        return torch.randn(c, device="cuda", generator=g)

    return rnd() * 0.2, rnd().abs() * 0.3 + 0.8, rnd() * 0.5 + 1.0, rnd() * 0.5


def _rand_x(shape, dtype, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return _cl(torch.randn(*shape, device="cuda", generator=g).to(dtype))


def _new_forward(x, mean, invstd, gamma, beta):
    from horovod_amd import _core
    n, c, h, w = x.shape
    oh, ow = _pooled_hw(h, w)
    pooled = _cl(torch.empty(n, c, oh, ow, device="cuda", dtype=x.dtype))
    codes = _cl(torch.empty(n, c, oh, ow, device="cuda", dtype=torch.uint8))
    _core.fused_bn_pool_pass(0, x, pooled, codes, None, mean, invstd, gamma,
                             beta)
    return pooled, codes


def _old_forward(x, mean, invstd, gamma, beta):
    from horovod_amd import _core
    y = torch.empty_like(x)
    _core.fused_bn_pass(1, x, None, None, y, mean, invstd, gamma, beta)
    ref, idx = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    return y, ref, idx


def _check_forward(x, stats):
    pooled, codes = _new_forward(x, *stats)
    y, ref, idx = _old_forward(x, *stats)
    assert pooled.shape == ref.shape
    assert int(codes.max()) <= 8
    assert torch.equal(_bits(pooled), _bits(_cl(ref)))
    assert torch.equal(_flat_index(codes, *x.shape[2:]), idx)
    assert torch.equal(torch.isnan(pooled), torch.isnan(ref))
    return pooled, codes, y, idx


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_is_bit_equal(case):
    shape, dtype = case
    _check_forward(_rand_x(shape, dtype, 1), _stats(shape[1], 2))


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_ties(case):
    """x from four distinct values, so nearly every window has a tie and the
    first maximum in ATen's scan order has to win; channel 0 is negative
    before the ReLU everywhere, so each of its windows is all zero."""
    shape, dtype = case
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    values = torch.tensor([-1.0, 0.0, 0.5, 1.0], device="cuda")
    x = _cl(values[torch.randint(0, 4, shape, device="cuda",
                                 generator=g)].to(dtype))
    mean, invstd, gamma, beta = _stats(shape[1], 4)
    beta[0] = -100.0
    pooled, codes, y, idx = _check_forward(x, (mean, invstd, gamma, beta))
    assert float(y[:, 0].abs().max()) == 0.0
    assert float(pooled[:, 0].abs().max()) == 0.0
    if shape[2] > 2:
        # windows with a tie for the maximum
        win = F.unfold(y.float(), 3, padding=1, stride=2).view(
            shape[0], shape[1], 9, -1)
        ties = ((win == win.max(dim=2, keepdim=True).values).sum(2) > 1)
        print(f"{_id(case)}: {int(ties.sum())} of {ties.numel()} windows tie")
        assert int(ties.sum()) > ties.numel() // 4


@requires_gpu
def test_forward_nan_and_inf():
    """NaN and +-inf in x.  The fused ReLU is f > 0 ? f : 0, which stores 0
    for a NaN pre-activation in the existing pass and in the pooled one
    alike, so no NaN reaches the pool on either side: this checks that the
    two agree on such input (and on +inf, which does reach the pool), not the
    NaN term of the pool's update rule, which no input can reach."""
    shape, dtype = SHAPES[2], torch.bfloat16
    x = _rand_x(shape, dtype, 5)
    x[0, 3, 4, 5] = float("nan")
    x[0, 9, 0, 0] = float("nan")
    x[0, 17, 8, 9] = float("inf")
    x[0, 20, 2, 2] = float("-inf")
    mean, invstd, gamma, beta = _stats(shape[1], 6)
    gamma = gamma.abs() + 0.1  # +inf stays +inf
    pooled, _, y, _ = _check_forward(x, (mean, invstd, gamma, beta))
    ref = F.max_pool2d(y, 3, 2, 1)
    assert torch.equal(torch.isnan(pooled), torch.isnan(ref))
    assert int(torch.isinf(pooled).sum()) > 0


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_is_exact(case):
    """Integer-valued gp in [-8, 8]: a sum of up to four of them is exact in
    every dtype, so the gathered fp32 gradient equals ATen's rounded one and
    the new backward apply must reproduce the existing one bit for bit.

    The stats pass: sum(g) is a sum of integers, exact in any order, and is
    compared exactly.  sum(g * xhat) is held to rtol 1e-5 of the fp64 sum of
    the same products wherever that sum does not cancel (|sum| >=
    sum|.| / 16), and to 1e-5 of sum|.| / 16 where it does: the order of an
    fp32 sum moves it by about sqrt(80 additions) * 2^-24 * sum|.| = 5e-7
    sum|.|, which rtol 1e-5 of a smaller sum cannot allow for.  The existing
    pass on ATen's dy is held to the same."""
    from horovod_amd import _core
    shape, dtype = case
    n, c, h, w = shape
    x = _rand_x(shape, dtype, 7)
    mean, invstd, gamma, beta = _stats(c, 8)
    pooled, codes = _new_forward(x, mean, invstd, gamma, beta)
    y, ref, idx = _old_forward(x, mean, invstd, gamma, beta)
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    gp = _cl(torch.randint(-8, 9, pooled.shape, device="cuda",
                           generator=g).to(dtype))
    dy = _cl(torch.ops.aten.max_pool2d_with_indices_backward(
        gp, y, [3, 3], [2, 2], [1, 1], [1, 1], False, idx))

    # apply: sums = (mean, invstd), as pass 5 of fused_bn_pass has them
    dx_new = torch.empty_like(x)
    _core.fused_bn_pool_pass(2, x, gp, codes, dx_new, mean, invstd, gamma,
                             beta, mean, invstd)
    dx_old = torch.empty_like(x)
    _core.fused_bn_pass(5, x, None, dy, dx_old, mean, invstd, gamma, beta)
    assert torch.equal(_bits(dx_new), _bits(dx_old))

    # stats
    banks = _core.fused_bn_pool_pass(1, x, gp, codes, None, mean, invstd,
                                     gamma, beta)
    assert banks.shape == (64, 2 * c)
    folded = banks.sum(0)
    old = _core.fused_bn_relu_backward(x, None, dy, mean, invstd, gamma,
                                       False, beta)
    gd = torch.where(y > 0, dy, torch.zeros_like(dy)).double()
    # the kernel's own fp32 x - mean and its one product with invstd
    xc = (x.float() - mean[None, :, None, None]).double()
    prod = gd * xc * invstd.double()[None, :, None, None]
    sum_g = gd.sum(dim=(0, 2, 3))
    sum_gx = prod.sum(dim=(0, 2, 3))
    scale = prod.abs().sum(dim=(0, 2, 3))
    strict = sum_gx.abs() >= scale / 16
    bound = 1e-5 * torch.where(strict, sum_gx.abs(), scale / 16)
    for name, got_g, got_gx in (("new", folded[:c], folded[c:]),
                                ("existing", old[2], old[1])):
        err = (got_gx.double() - sum_gx).abs()
        rel_sum = (err / sum_gx.abs().clamp_min(1e-30))[strict]
        print(f"{_id(case)} {name}: sum(g) max err "
              f"{_err(got_g, sum_g):.3g}; sum(g xhat): {int(strict.sum())} of "
              f"{c} channels at rtol of the sum, max rel err "
              f"{float(rel_sum.max()) if rel_sum.numel() else 0.0:.3g}; "
              f"all channels max err / sum|.| "
              f"{float((err / scale.clamp_min(1e-30)).max()):.3g}")
        assert torch.equal(got_g.double(), sum_g), name
        assert bool((err <= bound).all()), name


# ---- end to end --------------------------------------------------------------

def _module(c, gamma, beta):
    from horovod_amd.ops import FusedBNReLU
    m = FusedBNReLU(c, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        m.weight.copy_(gamma)
        m.bias.copy_(beta)
    return m


def _e2e_inputs(shape, dtype):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    n, c, h, w = shape
    x = _cl(torch.randn(*shape, device="cuda", generator=g).to(dtype))
    gp = _cl(torch.randn(n, c, *_pooled_hw(h, w), device="cuda",
                         generator=g).to(dtype))
    gamma = torch.randn(c, device="cuda", generator=g) * 0.5 + 1.0
    beta = torch.randn(c, device="cuda", generator=g) * 0.5
    return x, gp, gamma, beta


def _e2e_reference(x, gp, gamma, beta, pooled, codes):
    """fp64 forward composite, and the backward routed as the fused forward
    routed it (see the module docstring)."""
    n, c, h, w = x.shape
    xd = x.double()
    cnt = xd.numel() // c
    rm0, rv0 = torch.zeros(c, device="cuda", dtype=torch.float64), \
        torch.ones(c, device="cuda", dtype=torch.float64)
    y = F.relu(F.batch_norm(xd, rm0, rv0, gamma.double(), beta.double(), True,
                            MOMENTUM, EPS))
    pooled_ref = F.max_pool2d(y, 3, 2, 1)
    mean = xd.mean(dim=(0, 2, 3))
    var = xd.var(dim=(0, 2, 3), unbiased=False)
    invstd = (var + EPS).rsqrt()
    xhat = (xd - mean[None, :, None, None]) * invstd[None, :, None, None]
    live = torch.where(pooled > 0, gp, torch.zeros_like(gp)).double()
    g = torch.zeros(n, c, h * w, device="cuda", dtype=torch.float64)
    g.scatter_add_(2, _flat_index(codes, h, w).view(n, c, -1),
                   live.reshape(n, c, -1))
    g = g.view(n, c, h, w)
    sum_g = g.sum(dim=(0, 2, 3))
    sum_gx = (g * xhat).sum(dim=(0, 2, 3))
    dx = (gamma.double() * invstd)[None, :, None, None] * (
        g - (sum_g / cnt)[None, :, None, None] -
        xhat * (sum_gx / cnt)[None, :, None, None])
    return pooled_ref, dx, sum_gx, sum_g, rm0, rv0


def _e2e_check(shape, dtype, run=None):
    """One forward and backward of forward_maxpool against the reference.
    run(m, pool, xg, gp) -> (pooled, codes, dx, dgamma, dbeta), default
    eager."""
    from horovod_amd.ops.fused_bn import _FusedBNReLUPoolFn
    x, gp, gamma, beta = _e2e_inputs(shape, dtype)
    m = _module(shape[1], gamma, beta)
    pool = torch.nn.MaxPool2d(3, stride=2, padding=1)

    def eager(m, pool, xg, gp):
        pooled = m.forward_maxpool(xg, pool)
        assert isinstance(pooled.grad_fn, _FusedBNReLUPoolFn._backward_cls)
        codes = pooled.grad_fn.saved_tensors[1]
        dx, dgamma, dbeta = torch.autograd.grad(
            pooled, (xg, m.weight, m.bias), gp)
        return pooled.detach(), codes, dx, dgamma, dbeta

    xg = x.clone().requires_grad_(True)
    pooled, codes, dx, dgamma, dbeta = (run or eager)(m, pool, xg, gp)
    torch.cuda.synchronize()
    tol = TOL[dtype]
    p_ref, dx_ref, dgamma_ref, dbeta_ref, rm, rv = _e2e_reference(
        x, gp, gamma, beta, pooled, codes)
    tag = _id((shape, dtype))
    print(f"{tag}: pooled {_err(pooled, p_ref):.3g} dx {_err(dx, dx_ref):.3g}"
          f" dgamma {_err(dgamma, dgamma_ref):.3g} dbeta "
          f"{_err(dbeta, dbeta_ref):.3g}")
    assert _close(pooled, p_ref, tol), tag
    assert _close(dx, dx_ref, tol), tag
    assert _close(dgamma, dgamma_ref, 1e-2), tag
    assert _close(dbeta, dbeta_ref, 1e-2), tag
    return m, rm, rv, (pooled, dx, dgamma, dbeta)


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_module_matches_fp64_composite(case):
    shape, dtype = case
    m, rm, rv, _ = _e2e_check(shape, dtype)
    assert torch.allclose(m.running_mean.double(), rm, atol=1e-4)
    assert torch.allclose(m.running_var.double(), rv, atol=1e-3)


_CHILD_WORKSPACE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import test_gpu_fused_bn_pool as t
from horovod_amd import _core
assert not _core.fused_bn_lean_path()
assert _core.fused_bn_pool_path()
for shape in (t.SHAPES[0], t.SHAPES[2]):
    m, rm, rv, _ = t._e2e_check(shape, torch.bfloat16)
    assert torch.allclose(m.running_mean.double(), rm, atol=1e-4)
    assert torch.allclose(m.running_var.double(), rv, atol=1e-3)
print("CHILD_OK")
"""


def _child(code, env_extra, *argv):
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, "-c", code, os.path.join(ROOT, "tests"), *argv],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


@requires_gpu
def test_module_with_per_call_banks():
    """HOROVOD_FUSED_BN_WORKSPACE=0 is read once per process, so a fresh
    child runs the end-to-end check with per-call banks and their memset."""
    out = _child(_CHILD_WORKSPACE, {"HOROVOD_FUSED_BN_WORKSPACE": "0"})
    assert "CHILD_OK" in out, out[-2000:]


@requires_gpu
def test_module_in_a_captured_graph():
    """Forward and backward captured once and replayed three times: every
    replay meets the reference and the eager run's results (the stats sums
    are atomic, so not bit for bit)."""
    shape, dtype = SHAPES[2], torch.bfloat16
    _, _, _, eager = _e2e_check(shape, dtype)
    replays = []

    def run(m, pool, xg, gp):
        def fwd_bwd():
            pooled = m.forward_maxpool(xg, pool)
            codes = pooled.grad_fn.saved_tensors[1]
            grads = torch.autograd.grad(pooled, (xg, m.weight, m.bias), gp)
            return (pooled.detach(), codes) + tuple(grads)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = fwd_bwd()
        for _ in range(3):
            for t in static:
                if t.is_floating_point():
                    t.fill_(float("nan"))
                else:
                    t.fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            replays.append([t.clone() for t in static])
        return static

    _e2e_check(shape, dtype, run)
    tol = TOL[dtype]
    assert len(replays) == 3
    for rep in replays:
        pooled, codes, dx, dgamma, dbeta = rep
        assert int(codes.max()) <= 8
        assert _close(pooled, eager[0].double(), tol)
        assert _close(dx, eager[1].double(), tol)
        assert _close(dgamma, eager[2].double(), 1e-2)
        assert _close(dbeta, eager[3].double(), 1e-2)


@requires_gpu
def test_fallbacks_match_the_stock_ops():
    """Eval mode, a planar input, a MaxPool2d(2, 2) and a ceil_mode pool run
    BN+ReLU and the pool as two ops, and match stock nn.BatchNorm2d + relu +
    pool: bit for bit where BN itself is the stock op (eval, planar), within
    the fp32 tolerance where it is the fused BN+ReLU pass."""
    import copy
    from horovod_amd.ops.fused_bn import _FusedBNReLUPoolFn
    shape, dtype = SHAPES[1], torch.float32
    x, _, gamma, beta = _e2e_inputs(shape, dtype)
    pool321 = torch.nn.MaxPool2d(3, stride=2, padding=1)
    cases = [("eval", x, pool321, False),
             ("planar", x.contiguous(), pool321, True),
             ("pool 2/2", x, torch.nn.MaxPool2d(2, 2), True),
             ("ceil_mode", x, torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True),
              True)]
    for name, inp, pool, training in cases:
        m = _module(shape[1], gamma, beta).train(training)
        stock = torch.nn.BatchNorm2d(shape[1], eps=EPS,
                                     momentum=MOMENTUM).cuda().train(training)
        stock.load_state_dict(copy.deepcopy(m.state_dict()))
        xg = inp.clone().requires_grad_(True)
        xs = inp.clone().requires_grad_(True)
        got = m.forward_maxpool(xg, pool)
        exp = pool(F.relu(stock(xs)))
        assert not isinstance(got.grad_fn, _FusedBNReLUPoolFn._backward_cls), \
            name
        if name in ("eval", "planar"):
            assert torch.equal(got, exp), name
        else:
            assert _close(got, exp.double(), TOL[dtype]), name
        assert torch.allclose(m.running_mean, stock.running_mean,
                              atol=1e-4), name
        assert torch.allclose(m.running_var, stock.running_var,
                              atol=1e-3), name
        got.sum().backward()
        exp.sum().backward()
        assert _close(xg.grad, xs.grad.double(), TOL[dtype]), name
        assert _close(m.weight.grad, stock.weight.grad.double(), 1e-2), name


# ---- the model -------------------------------------------------------------

def _model_two_steps():
    """Two SGD steps of resnet50(num_classes=10) under bf16 autocast on fixed
    data, observed through model(...) itself -> (the grad_fn names of
    layer1's input, one per forward; how often model.maxpool ran;
    [loss, loss])."""
    from horovod_amd.models import resnet50
    torch.manual_seed(5)
    model = resnet50(num_classes=10).cuda().to(
        memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    data = _cl(torch.randn(4, 3, 64, 64, device="cuda", generator=g))
    target = torch.tensor([1, 7, 3, 0], device="cuda")
    names, pool_calls = [], []
    model.layer1.register_forward_pre_hook(
        lambda mod, args: names.append(type(args[0].grad_fn).__name__))
    model.maxpool.register_forward_hook(
        lambda mod, args, out: pool_calls.append(1))
    losses = []
    for _ in range(2):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(model(data), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return names, len(pool_calls), losses


_CHILD_MODEL = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import test_gpu_fused_bn_pool as t
from horovod_amd import _core
assert not _core.fused_bn_pool_path()
print("RESULT " + json.dumps(t._model_two_steps()))
"""


@requires_gpu
def test_model_takes_the_pooled_path():
    """model(data) of resnet50 feeds layer1 from the pooled autograd Function
    and never runs model.maxpool; a process with HOROVOD_FUSED_BN_POOL=0 runs
    model.maxpool once per forward and feeds layer1 from its backward node.
    Two steps of the two give the same losses within the bf16 tolerance
    test_gpu_fused_bn_workspace.py uses for its two paths (5e-2, rtol =
    atol)."""
    import json
    names, pool_calls, losses = _model_two_steps()
    assert len(names) == 2 and \
        all(n.startswith("_FusedBNReLUPoolFn") for n in names), names
    assert pool_calls == 0
    out = _child(_CHILD_MODEL, {"HOROVOD_FUSED_BN_POOL": "0"})
    line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
    off_names, off_pool_calls, off_losses = json.loads(line[len("RESULT "):])
    assert len(off_names) == 2 and \
        all("MaxPool" in n for n in off_names), off_names
    assert off_pool_calls == 2
    print("pooled path losses", losses, "two-op path losses", off_losses)
    assert all(torch.isfinite(torch.tensor(losses + off_losses)))
    tol = TOL[torch.bfloat16]
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64),
                          torch.tensor(off_losses, dtype=torch.float64),
                          rtol=tol, atol=tol)
