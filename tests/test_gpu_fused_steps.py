"""GPU tests (MI355X) that call the SGD and AdamW step kernels directly
through _core.fused_sgd_step / _core.fused_adamw_step
(csrc/sgd_kernels.hip, csrc/adamw_kernels.hip, host side in
csrc/multi_tensor.cc).

The reference is an fp64 evaluation of torch.optim.SGD's / AdamW's
definition written here, independent of fused_sgd.py and fused_adamw.py.
Inputs are those of the LAMB kernel tests (test_gpu_lamb.py): the edge list
and the 100-tensor list that crosses the 48-descriptor capacity twice.
Tolerances are the project's rtol=1e-5, atol=1e-6: on these seeded inputs an
fp32 torch evaluation of the same formulas, on the CPU, uses at most 0.044
of that bound for the SGD variants and 0.11 for AdamW (worst |err| / (atol +
rtol * |ref|) over all outputs, with and without the coefficient).
"""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

RTOL, ATOL = 1e-5, 1e-6

SGD_VARIANTS = {
    "plain": dict(lr=0.1, momentum=0.0, weight_decay=0.01, dampening=0.0,
                  nesterov=False),
    "momentum_dampening": dict(lr=0.1, momentum=0.9, weight_decay=0.01,
                               dampening=0.1, nesterov=False),
    "nesterov": dict(lr=0.1, momentum=0.9, weight_decay=0.01, dampening=0.0,
                     nesterov=True),
}
ADAMW = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
ADAMW_STEPS = [1, 7]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    yield


# ---- inputs: (p, g, m, v) per tensor; SGD uses m as its momentum buffer ----

def _randn(shape, seed, scale=1.0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def _tuple(n, seed, scale=1.0, offset=0, dev="cuda"):
    """offset=1 makes views that are not 16-byte aligned."""
    def mk(s, sc):
        return _randn((n + offset,), s, sc, dev)[offset:]
    return [mk(seed, scale), mk(seed + 1, 1.0), mk(seed + 2, 0.1),
            mk(seed + 3, 0.1).square_()]


def edge_tuples(dev="cuda"):
    ts = [_tuple(n, 10 * n, sc, dev=dev) for n, sc in
          [(0, 1.0), (1, 20.0), (3, 0.05), (33, 1.0), (4097, 20.0)]]
    ts.append(_tuple(1029, 7, 0.05, offset=1, dev=dev))
    if dev == "cuda":
        assert all(t.data_ptr() % 16 != 0 for t in ts[-1])
    ts.append(_tuple(20000, 8, dev=dev))
    ts.append([_randn((100,), 11, dev=dev)] +      # g = m = v = 0
              [torch.zeros(100, device=dev) for _ in range(3)])
    return ts


def many_tuples(dev="cuda"):
    """100 tensors of 5..40 elements: crosses the 48-descriptor capacity
    twice."""
    return [_tuple(5 + (7 * i) % 36, 200 + 4 * i, (0.05, 1.0, 20.0)[i % 3],
                   dev=dev)
            for i in range(100)]


LISTS = {"edge": edge_tuples, "capacity": many_tuples}


def _copy(tuples):
    return [[x.clone() for x in t] for t in tuples]


# ---- the definitions, in the dtype of what they are given ------------------

def sgd_definition(t, coef, lr, momentum, weight_decay, dampening, nesterov):
    """-> (p, momentum buffer) after one torch.optim.SGD step from a given
    buffer."""
    p, g, m = t[0], t[1] * coef, t[2]
    d = g + weight_decay * p
    if momentum != 0:
        m = momentum * m + (1 - dampening) * d
        d = d + momentum * m if nesterov else m
    return p - lr * d, m


def adamw_definition(t, coef, step, lr, beta1, beta2, eps, weight_decay):
    """-> (p, exp_avg, exp_avg_sq) after torch.optim.AdamW's step `step`."""
    p, g, m, v = t[0], t[1] * coef, t[2], t[3]
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p * (1 - lr * weight_decay) - (lr / bc1) * m / denom, m, v


def _close(got, want, where):
    got = got.double()
    assert torch.allclose(got, want, rtol=RTOL, atol=ATOL), \
        (where, (got - want).abs().max().item())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _sgd_call(tuples, kw, grad_coef=None):
    from horovod_amd import _core
    _core.fused_sgd_step([t[0] for t in tuples], [t[1] for t in tuples],
                         [t[2] for t in tuples] if kw["momentum"] else [],
                         kw["lr"], kw["momentum"], kw["weight_decay"],
                         kw["dampening"], kw["nesterov"], grad_coef)


def _adamw_call(tuples, step, grad_coef=None):
    from horovod_amd import _core
    _core.fused_adamw_step([t[0] for t in tuples], [t[1] for t in tuples],
                           [t[2] for t in tuples], [t[3] for t in tuples],
                           ADAMW["lr"], ADAMW["beta1"], ADAMW["beta2"],
                           ADAMW["eps"], ADAMW["weight_decay"], step,
                           grad_coef)


def _check(before, call, definition, n_out):
    """One step without and with grad_coef=0.25 against `definition` in
    fp64; the 0.25 run bitwise against gradients scaled beforehand."""
    coef = torch.full((1,), 0.25, device="cuda")
    for c in (None, coef):
        got = _copy(before)
        call(got, c)
        for i, (t, b) in enumerate(zip(got, before)):
            assert _same_bits(t[1], b[1]), "gradients are only read"
            want = definition([x.double() for x in b],
                              1.0 if c is None else 0.25)
            for k, w in zip((0, 2, 3)[:n_out], want):
                _close(t[k], w, (i, k, c is not None))
            for k in (2, 3)[n_out - 1:]:
                assert _same_bits(t[k], b[k]), "unused state is untouched"
    pre = _copy(before)
    for t in pre:
        t[1] = t[1] * 0.25
    call(pre, None)
    for i, (t, s) in enumerate(zip(got, pre)):
        for k in (0, 2, 3):
            assert _same_bits(t[k], s[k]), (i, k)
    # the step did something
    assert not torch.equal(got[-1][0], before[-1][0])


@requires_gpu
@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("variant", list(SGD_VARIANTS))
def test_sgd_kernel_vs_fp64(variant, which):
    kw = SGD_VARIANTS[variant]
    _check(LISTS[which](),
           lambda tuples, c: _sgd_call(tuples, kw, c),
           lambda t, coef: sgd_definition(t, coef, **kw),
           2 if kw["momentum"] else 1)


@requires_gpu
@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("step", ADAMW_STEPS)
def test_adamw_kernel_vs_fp64(step, which):
    _check(LISTS[which](),
           lambda tuples, c: _adamw_call(tuples, step, c),
           lambda t, coef: adamw_definition(t, coef, step, **ADAMW),
           3)


# ---- rejection -------------------------------------------------------------

def _rejects(call, ok):
    """LAMB's bad inputs (test_gpu_lamb.py): each raises before any launch."""
    keep = ok[0].clone()
    p, g, rest = ok[0], ok[1], ok[2:]
    with pytest.raises(RuntimeError, match="fp32"):
        call([p], [g.half()], *[[x] for x in rest])
    with pytest.raises(RuntimeError, match="GPU"):
        call([p], [g.cpu()], *[[x] for x in rest])
    with pytest.raises(RuntimeError, match="size"):
        call([p], [g[:7]], *[[x] for x in rest])
    with pytest.raises(RuntimeError, match="dense"):
        call([p], [_randn((16,), 2)[::2]], *[[x] for x in rest])
    with pytest.raises(RuntimeError, match="as many"):
        call([p], [], *[[x] for x in rest])
    assert _same_bits(ok[0], keep), "a rejected call must not launch"
    call(*[[] for _ in ok])                      # empty lists: a no-op


@requires_gpu
def test_sgd_kernel_rejects_bad_inputs():
    from horovod_amd import _core
    _rejects(lambda p, g, m: _core.fused_sgd_step(
        p, g, m, 0.1, 0.9, 0.01, 0.0, False, None), _tuple(8, 1)[:3])


@requires_gpu
def test_adamw_kernel_rejects_bad_inputs():
    from horovod_amd import _core
    _rejects(lambda p, g, m, v: _core.fused_adamw_step(
        p, g, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.05, 3, None), _tuple(8, 1))


# ---- a gradient laid out unlike its parameter -------------------------------

@requires_gpu
def test_mismatched_gradient_layout_takes_eager_update():
    """The kernels walk memory order, so a contiguous gradient of a
    channels_last parameter goes to the eager update (with the warning); the
    momentum buffer it leaves has the parameter's layout, and a later
    gradient in that layout takes the kernel."""
    from horovod_amd.ops import FusedSGD
    shape = (8, 4, 3, 3)
    p = _randn(shape, 60).to(memory_format=torch.channels_last)
    p.requires_grad_(True)
    q = p.detach().clone().requires_grad_(True)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01)
    opt, ref = FusedSGD([p], **kw), torch.optim.SGD([q], **kw)
    for step in range(4):
        g = _randn(shape, 61 + step)
        assert g.is_contiguous() and not p.is_contiguous()
        q.grad = g.clone()
        if step == 0:
            p.grad = g.clone()
            with pytest.warns(UserWarning, match="FusedSGD.*eager"):
                opt.step()
        else:
            p.grad = g.clone() if step == 1 else \
                g.to(memory_format=torch.channels_last)
            assert (p.grad.stride() == p.stride()) == (step > 1)
            opt.step()
        ref.step()
        assert opt.state[p]["momentum_buffer"].stride() == p.stride()
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
            (step, (p - q).abs().max().item())


# ---- state dict of torch.optim.AdamW ---------------------------------------

@requires_gpu
def test_fused_adamw_continues_torch_adamw_state_dict():
    """torch.optim.AdamW keeps `step` as a tensor; FusedAdamW loads that
    state dict and follows torch from there, on the kernels."""
    from horovod_amd.ops import FusedAdamW
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    shapes = [(33,), (128, 64), (7, 3, 3), (1029,)]
    ps = [_randn(s, 40 + i).requires_grad_(True)
          for i, s in enumerate(shapes)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    ref = torch.optim.AdamW(qs, **kw)

    def feed(step):
        for i, (p, q) in enumerate(zip(ps, qs)):
            q.grad = _randn(p.shape, 100 * step + i)
            p.grad = q.grad.clone()

    for step in range(2):
        feed(step)
        ref.step()
    assert torch.is_tensor(ref.state[qs[0]]["step"])
    for p, q in zip(ps, qs):
        p.data.copy_(q.data)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no eager fallback here
        opt = FusedAdamW(ps, **kw)
        # a copy, as if saved and loaded: load_state_dict keeps the step
        # tensor it is given, and ref goes on counting in its own
        opt.load_state_dict(copy.deepcopy(ref.state_dict()))
        assert torch.is_tensor(opt.state[ps[0]]["step"])
        for step in range(2, 5):
            feed(step)
            ref.step()
            opt.step()
            for i, (p, q) in enumerate(zip(ps, qs)):
                assert int(opt.state[p]["step"]) == step + 1
                assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
                    (step, i, (p - q).abs().max().item())
