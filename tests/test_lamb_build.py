"""FusedLAMB: the native surface exists after build() and the optimizer
follows its definition on CPU parameters through the eager path (no GPU
needed).

The reference is an independent fp64 evaluation of the definition in
docs/api.md, written here with plain per-tensor torch ops.  Tolerances are
those of test_fused_adamw_matches_torch: an fp32 eager evaluation of the
definition stays within them of the fp64 reference on these inputs (worst
absolute deviation 3.5e-6 after 6 steps, on the scale-10 tensor).
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers

SHAPES = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
SCALES = [0.02, 0.3, 3.0, 10.0, 1.0]
KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.01)
RTOL, ATOL = 1e-5, 1e-6
STEPS = 6


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * sc).requires_grad_(True)
            for s, sc in zip(SHAPES, SCALES)]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) for s in SHAPES]


class RefLamb:
    """The definition in fp64, one tensor at a time."""

    def __init__(self, params, lr, betas, eps, weight_decay,
                 bias_correction=True, always_adapt=False,
                 max_grad_norm=None):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = 0
        self.lr, (self.b1, self.b2), self.eps = lr, betas, eps
        self.wd, self.bc = weight_decay, bias_correction
        self.adapt = weight_decay != 0 or always_adapt
        self.max_grad_norm = max_grad_norm
        self.trust = []
        self.norm = None

    def step(self, grads):
        grads = [g.double() for g in grads]
        self.t += 1
        coef = 1.0
        if self.max_grad_norm is not None:
            self.norm = torch.sqrt(sum((g * g).sum() for g in grads)).item()
            coef = min(self.max_grad_norm / (self.norm + 1e-6), 1.0)
        self.trust = []
        for i, g in enumerate(grads):
            g = g * coef
            self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * g * g
            mhat, vhat = self.m[i], self.v[i]
            if self.bc:
                mhat = mhat / (1 - self.b1 ** self.t)
                vhat = vhat / (1 - self.b2 ** self.t)
            u = mhat / (vhat.sqrt() + self.eps) + self.wd * self.p[i]
            w_norm = self.p[i].norm().item()
            u_norm = u.norm().item()
            trust = 1.0
            if self.adapt and w_norm > 0 and u_norm > 0:
                trust = w_norm / u_norm
            self.trust.append(trust)
            self.p[i] = self.p[i] - self.lr * trust * u


def _follow(opt, ps, ref, steps=STEPS):
    for step in range(steps):
        grads = _grads(step)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(grads)
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g), "step() must not scale p.grad"
        for i, (p, q) in enumerate(zip(ps, ref.p)):
            assert torch.allclose(p.detach().double(), q, rtol=RTOL,
                                  atol=ATOL), \
                (step, i, (p.detach().double() - q).abs().max().item())


def test_core_exports_lamb_symbol():
    from horovod_amd import _core
    assert callable(getattr(_core, "fused_lamb_step", None))
    # validation comes before any launch: CPU tensors are an error, not a
    # quiet fallback
    t = [torch.ones(4) for _ in range(4)]
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_lamb_step([t[0]], [t[1]], [t[2]], [t[3]], 1e-3, 0.9,
                              0.999, 1e-6, 0.01, 1, True, True)
    assert torch.equal(t[0], torch.ones(4))


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_fused_lamb_matches_fp64_cpu(max_grad_norm):
    from horovod_amd.ops import FusedLAMB
    ps = _params()
    ref = RefLamb(ps, max_grad_norm=max_grad_norm, **KW)
    with pytest.warns(UserWarning, match="eager"):
        opt = FusedLAMB(ps, max_grad_norm=max_grad_norm, **KW)
        _follow(opt, ps, ref)
    # the inputs must make a wrong or missing trust ratio visible
    assert min(ref.trust) < 0.1 and max(ref.trust) > 5, ref.trust
    if max_grad_norm is None:
        assert opt.last_grad_norm is None
    else:
        assert ref.norm > 90, "clip must be active"
        assert opt.last_grad_norm.dim() == 0
        assert abs(opt.last_grad_norm.item() - ref.norm) <= 1e-5 * ref.norm


@pytest.mark.parametrize("extra", [dict(weight_decay=0.0, always_adapt=True),
                                   dict(weight_decay=0.0),
                                   dict(always_adapt=True),
                                   dict(bias_correction=False)],
                         ids=["wd0_adapt", "wd0", "adapt", "no_bias_corr"])
def test_options_follow_definition_cpu(extra):
    from horovod_amd.ops import FusedLAMB
    kw = dict(KW, **extra)
    ps = _params()
    ref = RefLamb(ps, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _follow(FusedLAMB(ps, **kw), ps, ref)
    if kw["weight_decay"] == 0 and not kw.get("always_adapt"):
        assert ref.trust == [1.0] * len(SHAPES)
    else:
        assert max(ref.trust) > 5


def test_wd0_without_adapt_is_adam_cpu():
    """weight_decay=0, always_adapt=False: every trust ratio is 1 and the
    update is Adam's, so torch.optim.Adam itself is the reference."""
    from horovod_amd.ops import FusedLAMB
    kw = dict(KW, weight_decay=0.0)
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
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


def test_invalid_options_raise():
    from horovod_amd.ops import FusedLAMB
    p = [torch.zeros(3, requires_grad=True)]
    for betas in [(1.0, 0.9), (0.9, 1.0), (-0.1, 0.9)]:
        with pytest.raises(ValueError, match="betas"):
            FusedLAMB(p, betas=betas)
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedLAMB(p, max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedLAMB([{"params": p, "max_grad_norm": bad}])


def test_differing_group_values_raise_at_step():
    from horovod_amd.ops import FusedLAMB
    a = torch.zeros(3, requires_grad=True)
    b = torch.zeros(3, requires_grad=True)
    for second in ({"max_grad_norm": 2.0}, {}):
        opt = FusedLAMB([{"params": [a], "max_grad_norm": 1.0},
                         dict(params=[b], **second)], lr=0.1)
        a.grad = torch.ones(3)
        b.grad = torch.ones(3)
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.step()


@pytest.mark.parametrize("source", ["torch", "fused"])
def test_adamw_state_dict_loads(source):
    """State keys are AdamW's: a run started under AdamW continues under
    FusedLAMB from its moments and step count."""
    from horovod_amd.ops import FusedAdamW, FusedLAMB
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        adamw = (torch.optim.AdamW if source == "torch" else FusedAdamW)(
            qs, lr=1e-2, betas=KW["betas"], eps=KW["eps"])
        grads = _grads(0)
        for q, g in zip(qs, grads):
            q.grad = g.clone()
        adamw.step()
        opt = FusedLAMB(ps, **KW)
        sd = adamw.state_dict()
        # the AdamW groups know nothing of LAMB's options
        for group in sd["param_groups"]:
            for key in ("bias_correction", "always_adapt"):
                assert key not in group
        opt.load_state_dict(sd)
        for group in opt.param_groups:
            assert group["bias_correction"] is True
            assert group["always_adapt"] is False
            assert group["max_grad_norm"] is None
            group.update(lr=KW["lr"], weight_decay=KW["weight_decay"])
        for p in ps:
            st = opt.state[p]
            assert int(st["step"]) == 1
            assert set(st) >= {"step", "exp_avg", "exp_avg_sq"}
        # second step: the reference takes its first on the same gradients,
        # then one more; the loaded optimizer must land where it does
        ref = RefLamb(ps, **KW)
        ref.step(grads)
        ref.p = [p.detach().double().clone() for p in ps]
        grads = _grads(1)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(grads)
    for i, (p, q) in enumerate(zip(ps, ref.p)):
        assert torch.allclose(p.detach().double(), q, rtol=RTOL, atol=ATOL), \
            (i, (p.detach().double() - q).abs().max().item())


DISTRIBUTED_BODY = """
        import warnings
        from horovod_amd.ops import FusedLAMB
        warnings.simplefilter("ignore")
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
        scales = [0.02, 0.3, 3.0, 10.0, 1.0]
        kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-5, weight_decay=0.02,
                  bias_correction=False, always_adapt=True,
                  max_grad_norm=1.0)

        def params(seed):
            g = torch.Generator().manual_seed(seed)
            return [(torch.randn(s, generator=g) * sc).requires_grad_(True)
                    for s, sc in zip(shapes, scales)]

        def grads(step):
            g = torch.Generator().manual_seed(100 + step)
            return [torch.randn(s, generator=g) for s in shapes]

        ps_w, ps_u = params(5), params(5)
        wrapped = hvd.DistributedOptimizer(FusedLAMB(ps_w, **kw))
        plain = FusedLAMB(ps_u, **kw)
        for group in wrapped.param_groups:
            for key, value in kw.items():
                assert group[key] == value, (key, group[key])
        for step in range(3):
            for p, q, g in zip(ps_w, ps_u, grads(step)):
                p.grad = g.clone()
                q.grad = g.clone()
            wrapped.step()
            plain.step()
            assert torch.equal(wrapped.last_grad_norm, plain.last_grad_norm)
            assert wrapped.last_grad_norm.item() > 90
        for p, q, p0 in zip(ps_w, ps_u, params(5)):
            assert torch.equal(p, q)
            assert not torch.equal(p, p0)
"""


def test_distributed_optimizer_keeps_lamb_options():
    """DistributedOptimizer rebuilds the optimizer from param_groups: every
    option, set to a non-default value here, must survive that, and the
    trajectory must be bitwise the unwrapped one.  Runs in a worker process
    so no initialised core outlives the test."""
    run_workers(1, DISTRIBUTED_BODY, timeout=120)
