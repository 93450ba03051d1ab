"""GPU tests (MI355X) for FusedLAMB and the three LAMB kernels
(csrc/lamb_kernels.hip): moments + norms, trust ratios, update.

The reference is the fp64 evaluation of the definition from
tests/test_lamb_build.py (RefLamb), independent of fused_lamb.py; inputs and
tolerances are the ones documented there.
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers
from tests.test_lamb_build import ATOL, KW, RTOL, STEPS, RefLamb
from tests.test_lamb_build import _grads as _cpu_grads
from tests.test_lamb_build import _params as _cpu_params

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    yield


def _params(seed=5):
    return [p.detach().cuda().requires_grad_(True) for p in _cpu_params(seed)]


def _grads(step):
    return [g.cuda() for g in _cpu_grads(step)]


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda()


def _close(p, q, where):
    p = p.detach().double()
    assert torch.allclose(p, q, rtol=RTOL, atol=ATOL, equal_nan=True), \
        (where, (p - q).abs().max().item())


def _follow(opt, ps, ref, steps=STEPS, grads_of=_grads, feed_ref=None):
    for step in range(steps):
        grads = grads_of(step)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(feed_ref(grads) if feed_ref else grads)
        for p, g in zip(ps, grads):
            # bitwise, so that a NaN put there on purpose compares equal
            assert torch.equal(p.grad.view(torch.int32),
                               g.view(torch.int32)), \
                "step() must not scale p.grad"
        for i, (p, q) in enumerate(zip(ps, ref.p)):
            _close(p, q, (step, i))


# ---- optimizer trajectories -----------------------------------------------

@requires_gpu
def test_fused_lamb_matches_fp64():
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    ref = RefLamb(ps, **KW)
    lo, hi = float("inf"), 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # no eager fallback here
        opt = FusedLAMB(ps, **KW)
        for step in range(STEPS):
            _follow(opt, ps, ref, steps=1, grads_of=lambda _: _grads(step))
            lo, hi = min(lo, *ref.trust), max(hi, *ref.trust)
    # a trust ratio of 1 everywhere would be far outside the tolerance
    assert lo < 0.1 and hi > 5, (lo, hi)


@requires_gpu
@pytest.mark.parametrize("extra", [dict(weight_decay=0.0, always_adapt=True),
                                   dict(always_adapt=True),
                                   dict(bias_correction=False)],
                         ids=["wd0_adapt", "adapt", "no_bias_corr"])
def test_options_follow_definition(extra):
    from horovod_amd.ops import FusedLAMB
    kw = dict(KW, **extra)
    ps = _params()
    _follow(FusedLAMB(ps, **kw), ps, RefLamb(ps, **kw), steps=3)


@requires_gpu
def test_wd0_without_adapt_is_adam():
    from horovod_amd.ops import FusedLAMB
    kw = dict(KW, weight_decay=0.0)
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    opt = FusedLAMB(ps, **kw)
    adam = torch.optim.Adam(qs, **kw)
    for step in range(STEPS):
        for p, q, g in zip(ps, qs, _grads(step)):
            p.grad = g.clone()
            q.grad = g.clone()
        opt.step()
        adam.step()
        for i, (p, q) in enumerate(zip(ps, qs)):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
                (step, i, (p - q).abs().max().item())


# ---- direct kernel calls --------------------------------------------------

HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-6, step=3,
             bias_correction=True, adapt=True)


def _tuple(n, seed, scale=1.0, offset=0):
    """(p, g, m, v) of n elements; offset=1 makes views that are not
    16-byte aligned."""
    def mk(s, sc):
        return _randn((n + offset,), s, sc)[offset:]
    return [mk(seed, scale), mk(seed + 1, 1.0), mk(seed + 2, 0.1),
            mk(seed + 3, 0.1).square_()]


def _edge_tuples():
    # parameter scales spread the ratios so a mixed-up index shows
    ts = [_tuple(n, 10 * n, sc) for n, sc in
          [(0, 1.0), (1, 20.0), (3, 0.05), (33, 1.0), (4097, 20.0)]]
    ts.append(_tuple(1029, 7, 0.05, offset=1))
    assert all(t.data_ptr() % 16 != 0 for t in ts[-1])
    ts.append(_tuple(20000, 8))          # three chunks, ragged last one
    zero_p = _tuple(100, 9)
    zero_p[0].zero_()                    # |p| = 0: trust 1, plain u
    ts.append(zero_p)
    ts.append([_randn((100,), 11)] +     # g = m = v = 0
              [torch.zeros(100, device="cuda") for _ in range(3)])
    return ts


def _many_tuples():
    """100 tensors of 5..40 elements: crosses the 48-descriptor capacity
    twice; the scales spread the ratios so a wrong index shows."""
    return [_tuple(5 + (7 * i) % 36, 200 + 4 * i, (0.05, 1.0, 20.0)[i % 3])
            for i in range(100)]


def _ref_direct(tuples, weight_decay, hyper=HYPER):
    ref = RefLamb([t[0] for t in tuples], hyper["lr"],
                  (hyper["beta1"], hyper["beta2"]), hyper["eps"],
                  weight_decay, bias_correction=hyper["bias_correction"])
    ref.adapt = hyper["adapt"]
    ref.m = [t[2].double() for t in tuples]
    ref.v = [t[3].double() for t in tuples]
    ref.t = hyper["step"] - 1
    ref.step([t[1] for t in tuples])
    return ref


def _torch_trust(t, weight_decay, hyper=HYPER):
    """The ratio formed with fp32 torch ops and vector_norm."""
    p, g, m, v = t
    b1, b2 = hyper["beta1"], hyper["beta2"]
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** hyper["step"])) / \
        ((v / (1 - b2 ** hyper["step"])).sqrt() + hyper["eps"]) + \
        weight_decay * p
    return (torch.linalg.vector_norm(p) / torch.linalg.vector_norm(u)).item()


def _call(tuples, weight_decay, hyper=HYPER, grad_coef=None):
    from horovod_amd import _core
    return _core.fused_lamb_step(
        [t[0] for t in tuples], [t[1] for t in tuples],
        [t[2] for t in tuples], [t[3] for t in tuples],
        weight_decay=weight_decay, grad_coef=grad_coef, **hyper)


def _check_direct(tuples, weight_decay, label):
    before = [[x.clone() for x in t] for t in tuples]
    ref = _ref_direct(before, weight_decay)
    trust = _call(tuples, weight_decay)
    assert trust.dtype == torch.float32 and trust.shape == (len(tuples),)
    assert trust.is_cuda
    trust = trust.tolist()
    worst = (0.0, 0.0)
    for i, (t, b) in enumerate(zip(tuples, before)):
        assert torch.equal(t[1], b[1]), "gradients are only read"
        _close(t[0], ref.p[i], (label, i, "p"))
        _close(t[2], ref.m[i], (label, i, "m"))
        _close(t[3], ref.v[i], (label, i, "v"))
        want = ref.trust[i]
        if want == 1.0:                  # the rule's 'otherwise' branch
            assert trust[i] == 1.0, (label, i, trust[i])
            continue
        err = abs(trust[i] - want) / want
        torch_err = abs(_torch_trust(b, weight_decay) - want) / want
        bound = max(4 * torch_err, 8 * 2.0 ** -23)
        worst = max(worst, (err, torch_err))
        assert err <= bound, (label, i, err, bound)
    print(f"trust[{label}, wd={weight_decay}]: worst native rel err "
          f"{worst[0]:.3e} (torch ops on that tensor {worst[1]:.3e})")
    return ref, trust


@requires_gpu
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_kernel_edge_list_vs_fp64(weight_decay):
    tuples = _edge_tuples()
    p_zero_grad = tuples[-1][0].clone()
    ref, trust = _check_direct(tuples, weight_decay, "edge")
    assert trust[0] == 1.0                       # empty tensor
    assert trust[-2] == 1.0                      # |p| = 0
    assert not any(torch.isnan(x).any() for t in tuples for x in t)
    if weight_decay == 0.0:
        # u = 0: trust 1 and the parameter is left as it was
        assert trust[-1] == 1.0
        assert torch.equal(tuples[-1][0], p_zero_grad)
    else:
        # u = weight_decay * p, so the ratio is 1 / weight_decay
        assert abs(trust[-1] - 100.0) < 1e-3
    assert min(ref.trust) < 0.5 and max(ref.trust) > 2, ref.trust


@requires_gpu
def test_kernel_100_tensors_vs_fp64():
    ref, trust = _check_direct(_many_tuples(), 0.01, "100_tensors")
    assert min(ref.trust) < 0.2 and max(ref.trust) > 5, ref.trust


@requires_gpu
def test_kernel_without_adapt_and_with_coef():
    """adapt=False gives trust 1 whatever the norms; a grad_coef of 0.25
    equals a gradient scaled by 0.25 beforehand."""
    hyper = dict(HYPER, adapt=False)
    tuples = [_tuple(n, 30 + n) for n in (33, 4097)]
    before = [[x.clone() for x in t] for t in tuples]
    ref = _ref_direct(before, 0.01, hyper)
    trust = _call(tuples, 0.01, hyper)
    assert trust.tolist() == [1.0, 1.0] and ref.trust == [1.0, 1.0]
    for i, t in enumerate(tuples):
        _close(t[0], ref.p[i], (i, "p"))

    coef = torch.full((1,), 0.25, device="cuda")
    a = [[x.clone() for x in t] for t in before]
    b = [[x.clone() for x in t] for t in before]
    for t in b:
        t[1] = t[1] * 0.25
    ta, tb = _call(a, 0.01, grad_coef=coef), _call(b, 0.01)
    assert torch.equal(ta, tb)
    for x, y, orig in zip(a, b, before):
        assert torch.equal(x[1], orig[1]), "gradients are only read"
        for k in (0, 2, 3):
            assert torch.equal(x[k], y[k])


@requires_gpu
def test_kernel_rejects_bad_inputs():
    from horovod_amd import _core
    ok = _tuple(8, 1)

    def call(p, g, m, v):
        _core.fused_lamb_step([p], [g], [m], [v], weight_decay=0.01, **HYPER)

    keep = ok[0].clone()
    with pytest.raises(RuntimeError, match="fp32"):
        call(ok[0], ok[1].half(), ok[2], ok[3])
    with pytest.raises(RuntimeError, match="GPU"):
        call(ok[0], ok[1].cpu(), ok[2], ok[3])
    with pytest.raises(RuntimeError, match="size"):
        call(ok[0], ok[1][:7], ok[2], ok[3])
    with pytest.raises(RuntimeError, match="dense"):
        call(ok[0], _randn((16,), 2)[::2], ok[2], ok[3])
    with pytest.raises(RuntimeError, match="as many"):
        _core.fused_lamb_step([ok[0]], [], [ok[2]], [ok[3]],
                              weight_decay=0.01, **HYPER)
    assert torch.equal(ok[0], keep), "a rejected call must not launch"
    assert _core.fused_lamb_step([], [], [], [], weight_decay=0.01,
                                 **HYPER).shape == (0,)


@requires_gpu
def test_kernel_deterministic():
    """No atomics: the same inputs give bitwise the same trust ratios and
    tensors, whatever the workspace held before."""
    base = _edge_tuples() + _many_tuples()
    runs = []
    for k in range(3):
        tuples = [[x.clone() for x in t] for t in base]
        runs.append((_call(tuples, 0.01), tuples))
        # the next call's workspace comes back from the caching allocator
        # with this call's partials, or with garbage, in it
        if k == 1:
            junk = torch.full((4096,), float("nan"), device="cuda")
            del junk
    for trust, tuples in runs[1:]:
        assert torch.equal(trust.view(torch.int32),
                           runs[0][0].view(torch.int32))
        for t, t0 in zip(tuples, runs[0][1]):
            for x, x0 in zip(t, t0):
                assert torch.equal(x, x0)


# ---- optimizer behaviour --------------------------------------------------

@requires_gpu
def test_nan_gradient_stays_in_its_tensor():
    """No clipping, so nothing global: a NaN in one gradient reaches only
    that tensor.  Its u_norm is NaN, the rule's compares are false, trust is
    1, and the NaN lands on the element it came from; every other tensor
    follows the reference."""
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    ref = RefLamb(ps, **KW)
    opt = FusedLAMB(ps, **KW)

    def grads_of(step):
        grads = _grads(step)
        if step == 1:
            grads[1][5, 7] = float("nan")
        return grads

    _follow(opt, ps, ref, steps=3, grads_of=grads_of)
    assert torch.isnan(ps[1][5, 7]) and torch.isnan(ref.p[1][5, 7])
    for i in (0, 2, 3, 4):
        assert not torch.isnan(ps[i]).any(), i


@requires_gpu
def test_clip_matches_reference_on_clipped_gradients():
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    ref = RefLamb(ps, **KW)
    opt = FusedLAMB(ps, max_grad_norm=1.0, **KW)
    norms = []

    def clipped(grads):
        qs = [torch.empty_like(g).requires_grad_(True) for g in grads]
        for q, g in zip(qs, grads):
            q.grad = g.clone()
        norms.append(torch.nn.utils.clip_grad_norm_(qs, 1.0))
        return [q.grad for q in qs]

    for step in range(STEPS):
        _follow(opt, ps, ref, steps=1, grads_of=lambda _: _grads(step),
                feed_ref=clipped)
        assert norms[-1].item() > 90, "clip must be active"
        assert opt.last_grad_norm.dim() == 0
        assert torch.allclose(opt.last_grad_norm, norms[-1], rtol=1e-5,
                              atol=0)


@requires_gpu
def test_inactive_clip_is_bitwise_noop():
    from horovod_amd.ops import FusedLAMB
    ps_c, ps_n = _params(), _params()
    oc = FusedLAMB(ps_c, max_grad_norm=1e4, **KW)
    on = FusedLAMB(ps_n, **KW)
    for step in range(3):
        for p, q, g in zip(ps_c, ps_n, _grads(step)):
            p.grad = g.clone()
            q.grad = g.clone()
        oc.step()
        on.step()
        for i, (p, q) in enumerate(zip(ps_c, ps_n)):
            assert torch.equal(p, q), (step, i, (p - q).abs().max().item())
    assert on.last_grad_norm is None
    assert 160 < oc.last_grad_norm.item() < 182     # sqrt(29312 elements)


@requires_gpu
def test_two_optimizers_bitwise_equal():
    from horovod_amd.ops import FusedLAMB
    ps_a, ps_b = _params(), _params()
    oa = FusedLAMB(ps_a, max_grad_norm=1.0, **KW)
    ob = FusedLAMB(ps_b, max_grad_norm=1.0, **KW)
    for step in range(3):
        for p, q, g in zip(ps_a, ps_b, _grads(step)):
            p.grad = g.clone()
            q.grad = g.clone()
        oa.step()
        junk = torch.full((4096,), float("nan"), device="cuda")
        del junk
        ob.step()
    for p, q, p0 in zip(ps_a, ps_b, _params()):
        assert torch.equal(p, q)
        assert not torch.equal(p, p0)
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)


@requires_gpu
def test_differing_steps_take_their_own_bias_correction():
    """Parameters restored mid-run can disagree on the step count."""
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    opt = FusedLAMB(ps, **KW)
    ref_a, ref_b = RefLamb(ps[:2], **KW), RefLamb(ps[2:], **KW)
    grads = _grads(0)
    for p, g in zip(ps[:2], grads[:2]):
        p.grad = g.clone()
    opt.step()                                  # ps[2:] have no gradient yet
    ref_a.step(grads[:2])
    grads = _grads(1)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt.step()
    ref_a.step(grads[:2])
    ref_b.step(grads[2:])
    assert [opt.state[p]["step"] for p in ps] == [2, 2, 1, 1, 1]
    for i, (p, q) in enumerate(zip(ps, ref_a.p + ref_b.p)):
        _close(p, q, i)


@requires_gpu
def test_mixed_eligibility_bf16_param():
    """A bf16 parameter among fp32 ones takes the eager update, the others
    the kernels.  The bf16 one is compared with the reference rounded to
    bf16.  Its moments are bf16 (relative error 2^-9 each), so u is off by
    about 2^-8 of an update of at most lr * |p| * 3 = 1e-3, which is 4e-6;
    rounding the result to bf16 adds half an ulp, 2^-9 relative.  Hence two
    ulp relative and 1e-5 absolute."""
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    ps[0] = ps[0].detach().to(torch.bfloat16).requires_grad_(True)
    grads = _grads(0)
    grads[0] = grads[0].to(torch.bfloat16)
    ref = RefLamb(ps, **KW)
    with pytest.warns(UserWarning, match="eager"):
        opt = FusedLAMB(ps, **KW)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
    ref.step(grads)
    assert ps[0].dtype == torch.bfloat16
    assert opt.state[ps[0]]["exp_avg"].dtype == torch.bfloat16
    want = ref.p[0].to(torch.bfloat16).float()
    assert torch.allclose(ps[0].detach().float(), want, rtol=2.0 ** -6,
                          atol=1e-5), \
        (ps[0].detach().float() - want).abs().max().item()
    assert not torch.equal(ps[0].detach(), _params()[0].to(torch.bfloat16))
    for i in range(1, len(ps)):
        _close(ps[i], ref.p[i], i)


# ---- two ranks ------------------------------------------------------------

TWO_RANK_BODY = """
        from horovod_amd import _core
        from horovod_amd.ops import FusedLAMB
        torch.cuda.set_device(hvd.local_rank() % torch.cuda.device_count())
        dev = torch.device("cuda",
                           hvd.local_rank() % torch.cuda.device_count())
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
        scales = [0.02, 0.3, 3.0, 10.0, 1.0]
        lr, b1, b2, eps, wd = 1e-2, 0.9, 0.95, 1e-6, 0.01

        def randn(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).to(dev) for s in shapes]

        ps = [(p * s).requires_grad_(True)            # same on all ranks
              for p, s in zip(randn(1), scales)]
        p0 = [p.detach().double().clone() for p in ps]
        per_rank = [randn(50 + r) for r in range(size)]
        opt = hvd.DistributedOptimizer(
            FusedLAMB(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd,
                      max_grad_norm=1.0),
            named_parameters=[(f"p{i}", p) for i, p in enumerate(ps)])
        assert all(g["max_grad_norm"] == 1.0 for g in opt.param_groups)
        for p, g in zip(ps, per_rank[rank]):
            p.grad = g.clone()
        opt.step()
        torch.cuda.synchronize()
        assert not _core.rccl_used(), "small gradients must stay one-shot"

        # the definition in fp64 on the mean gradient, first step
        mean = [(sum(gs) / size).double() for gs in zip(*per_rank)]
        norm = torch.sqrt(sum((g * g).sum() for g in mean)).item()
        assert norm > 10, "clip must be active"
        assert abs(opt.last_grad_norm.item() - norm) <= 1e-5 * norm
        coef = min(1.0 / (norm + 1e-6), 1.0)
        for p, w, gm in zip(ps, p0, mean):
            g = gm * coef
            mhat = (1 - b1) * g / (1 - b1)
            vhat = (1 - b2) * g * g / (1 - b2)
            u = mhat / (vhat.sqrt() + eps) + wd * w
            want = w - lr * (w.norm() / u.norm()) * u
            assert torch.allclose(p.detach().double(), want, rtol=1e-5,
                                  atol=1e-6), \\
                (p.detach().double() - want).abs().max().item()
            # the averaged gradient is left unscaled
            assert torch.allclose(p.grad.double(), gm, rtol=1e-6, atol=1e-7)
        # both ranks share one GPU, so the parameters travel as host tensors
        bits = torch.cat([p.detach().reshape(-1) for p in ps]).cpu()
        both = hvd.allgather(bits.view(torch.int32), name="lamb.param_bits")
        both = both.reshape(size, -1)
        assert bool((both == both[0]).all()), (both != both[0]).sum()
"""


@requires_gpu
def test_two_ranks_same_parameters():
    """Two ranks with different gradients take one clipped FusedLAMB step
    through hvd.DistributedOptimizer: parameters match the definition on the
    mean gradient and are bitwise the same on both ranks, with no collective
    for the trust ratios."""
    run_workers(2, TWO_RANK_BODY,
                extra_env={"HOROVOD_ONESHOT_ALLREDUCE": "1"}, timeout=300)
