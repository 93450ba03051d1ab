"""FusedLARS: the native surface exists after build() and the optimizer
follows its definition on CPU parameters through the eager path (no GPU
needed); split_decay_groups builds the two groups LARS is used with.

The reference is an independent fp64 evaluation of the definition in
docs/api.md, written here with plain per-tensor torch ops.  Inputs are those
of test_lamb_build.py.  Tolerances are those of
test_fused_adamw_matches_torch: an fp32 eager evaluation of the definition
stays within them of the fp64 reference on these inputs (worst absolute
deviation after 6 steps: plain 3.7e-6, nesterov 3.9e-6, trust_clip at
lr=0.05 3.6e-6, weight_decay=0 momentum=0 always_adapt 4.4e-6).
"""
import pickle
import warnings

import pytest
import torch

from tests.parallel_util import run_workers

SHAPES = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
SCALES = [0.02, 0.3, 3.0, 10.0, 1.0]
KW = dict(lr=1.0, momentum=0.9, weight_decay=0.01, trust_coefficient=0.02,
          eps=1e-8)
RTOL, ATOL = 1e-5, 1e-6
STEPS = 6


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * sc).requires_grad_(True)
            for s, sc in zip(SHAPES, SCALES)]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) for s in SHAPES]


class RefLars:
    """The definition in fp64, one tensor at a time."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0,
                 trust_coefficient=0.001, eps=1e-8, nesterov=False,
                 trust_clip=False, always_adapt=False, max_grad_norm=None):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.lr, self.mu, self.wd = lr, momentum, weight_decay
        self.tc, self.eps = trust_coefficient, eps
        self.nesterov, self.trust_clip = nesterov, trust_clip
        self.adapt = weight_decay != 0 or always_adapt
        self.max_grad_norm = max_grad_norm
        self.trust = []
        self.norm = None

    def step(self, grads):
        grads = [g.double() for g in grads]
        coef = 1.0
        if self.max_grad_norm is not None:
            self.norm = torch.sqrt(sum((g * g).sum() for g in grads)).item()
            coef = min(self.max_grad_norm / (self.norm + 1e-6), 1.0)
        self.trust = []
        for i, g in enumerate(grads):
            g = g * coef
            wn = self.p[i].norm().item()
            gn = g.norm().item()
            trust = 1.0
            if self.adapt and wn > 0 and gn > 0:
                trust = self.tc * wn / (gn + self.wd * wn + self.eps)
                if self.trust_clip:
                    trust = min(trust / self.lr, 1.0) if self.lr != 0 else 1.0
            self.trust.append(trust)
            d = trust * (g + self.wd * self.p[i])
            self.m[i] = self.mu * self.m[i] + d
            d = d + self.mu * self.m[i] if self.nesterov else self.m[i]
            self.p[i] = self.p[i] - self.lr * d


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


def check_spread(case, trust):
    """The reference's trust ratios on these inputs must make a wrong or
    missing ratio visible."""
    if case == "wd0":
        assert trust == [1.0] * len(SHAPES)
    elif case == "trust_clip":
        # two tensors clip to exactly 1, three stay adaptive
        assert sorted(trust)[3:] == [1.0, 1.0], trust
        assert all(0.01 < t < 0.5 for t in sorted(trust)[:3]), trust
    elif case == "clip":
        # gradients 170 times smaller: larger ratios, the weight-decay term
        # of the denominator caps them near trust_coefficient / weight_decay
        assert max(trust) > 10 * min(trust), trust
    else:
        assert min(trust) < 1e-3 and max(trust) > 0.1, trust


CASES = {
    "plain": {},
    "nesterov": dict(nesterov=True),
    "trust_clip": dict(trust_clip=True, lr=0.05),
    "wd0": dict(weight_decay=0.0),
    "wd0_adapt": dict(weight_decay=0.0, always_adapt=True),
    "wd0_mu0_adapt": dict(weight_decay=0.0, momentum=0.0, always_adapt=True),
    "clip": dict(max_grad_norm=1.0),
}


def test_core_exports_lars_symbol():
    from horovod_amd import _core
    assert callable(getattr(_core, "fused_lars_step", None))
    # validation comes before any launch: CPU tensors are an error, not a
    # quiet fallback
    t = [torch.ones(4) for _ in range(3)]
    with pytest.raises(RuntimeError, match="GPU"):
        _core.fused_lars_step([t[0]], [t[1]], [t[2]], 1.0, 0.9, 0.01, 0.02,
                              1e-8, False, False, True)
    assert torch.equal(t[0], torch.ones(4))


@pytest.mark.parametrize("case", list(CASES))
def test_fused_lars_matches_fp64_cpu(case):
    from horovod_amd.ops import FusedLARS
    kw = dict(KW, **CASES[case])
    ps = _params()
    ref = RefLars(ps, **kw)
    with pytest.warns(UserWarning, match="eager"):
        opt = FusedLARS(ps, **kw)
        _follow(opt, ps, ref)
    check_spread(case, ref.trust)
    if case == "clip":
        assert ref.norm > 90, "clip must be active"
        assert opt.last_grad_norm.dim() == 0
        assert abs(opt.last_grad_norm.item() - ref.norm) <= 1e-5 * ref.norm
    else:
        assert opt.last_grad_norm is None


def test_wd0_without_adapt_is_sgd_cpu():
    """weight_decay=0, always_adapt=False: every trust ratio is 1 and the
    update is momentum SGD's, so torch.optim.SGD itself is the reference."""
    from horovod_amd.ops import FusedLARS
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedLARS(ps, **dict(KW, weight_decay=0.0))
        sgd = torch.optim.SGD(qs, lr=KW["lr"], momentum=0.9)
        for step in range(STEPS):
            for p, q, g in zip(ps, qs, _grads(step)):
                p.grad = g.clone()
                q.grad = g.clone()
            opt.step()
            sgd.step()
            for i, (p, q) in enumerate(zip(ps, qs)):
                assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
                    (step, i, (p - q).abs().max().item())


def test_invalid_options_raise():
    from horovod_amd.ops import FusedLARS
    p = [torch.zeros(3, requires_grad=True)]
    for momentum in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            FusedLARS(p, lr=0.1, momentum=momentum)
    with pytest.raises(ValueError, match="nesterov"):
        FusedLARS(p, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="nesterov"):
        FusedLARS([{"params": p, "momentum": 0.0}], lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="trust_coefficient"):
        FusedLARS(p, lr=0.1, trust_coefficient=-0.001)
    with pytest.raises(TypeError):
        FusedLARS(p, lr=0.1, dampening=0.0)
    for bad in (0, -1.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedLARS(p, lr=0.1, max_grad_norm=bad)
    FusedLARS(p, lr=0.1, momentum=0.0)            # allowed: buffer is kept


def test_fused_sgd_state_dict_loads():
    """The state key is SGD's: a run started under FusedSGD continues under
    FusedLARS from its momentum buffer, and the group keys FusedSGD does not
    know take their defaults."""
    from horovod_amd.ops import FusedLARS, FusedSGD
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    grads = _grads(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sgd = FusedSGD(qs, lr=0.1, momentum=0.9)
        for q, g in zip(qs, grads):
            q.grad = g.clone()
        sgd.step()
        sd = sgd.state_dict()
        for group in sd["param_groups"]:
            for key in ("trust_coefficient", "eps", "trust_clip",
                        "always_adapt"):
                assert key not in group
        opt = FusedLARS(ps, **KW)
        opt.load_state_dict(sd)
        for group in opt.param_groups:
            assert group["trust_coefficient"] == 0.001
            assert group["eps"] == 1e-8
            assert group["trust_clip"] is False
            assert group["always_adapt"] is False
            assert group["max_grad_norm"] is None
            group.update(KW)
        # FusedSGD's first buffer is the gradient: the reference starts there
        ref = RefLars(ps, **KW)
        ref.m = [g.double() for g in grads]
        for p, g in zip(ps, grads):
            assert torch.equal(opt.state[p]["momentum_buffer"], g)
        grads = _grads(1)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(grads)
    for i, (p, q) in enumerate(zip(ps, ref.p)):
        assert torch.allclose(p.detach().double(), q, rtol=RTOL, atol=ATOL), \
            (i, (p.detach().double() - q).abs().max().item())


def test_torch_sgd_state_dict_before_first_step_loads():
    """torch.optim.SGD saves momentum_buffer=None until it has stepped."""
    from horovod_amd.ops import FusedLARS
    ps = _params()
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    sgd = torch.optim.SGD(qs, lr=0.1, momentum=0.9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedLARS(ps, **KW)
        opt.load_state_dict(sgd.state_dict())
        for group in opt.param_groups:
            group.update(KW)
        _follow(opt, ps, RefLars(ps, **KW), steps=2)


def test_pickle_round_trip():
    from horovod_amd.ops import FusedLARS
    kw = dict(KW, nesterov=True, trust_clip=True, always_adapt=True)
    ps = _params()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedLARS(ps, **kw)
        ref = RefLars(ps, **kw)
        _follow(opt, ps, ref, steps=2)
        opt = pickle.loads(pickle.dumps(opt))
        ps = [p for group in opt.param_groups for p in group["params"]]
        for group in opt.param_groups:
            for key, value in kw.items():
                assert group[key] == value, (key, group[key])
        assert opt.skipped_steps == 0 and opt.last_found_inf is None
        grads = _grads(2)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(grads)
    for i, (p, q) in enumerate(zip(ps, ref.p)):
        assert torch.allclose(p.detach().double(), q, rtol=RTOL, atol=ATOL), \
            (i, (p.detach().double() - q).abs().max().item())


def test_split_decay_groups():
    from horovod_amd.ops import FusedLARS, split_decay_groups
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3),
                              torch.nn.BatchNorm2d(4),
                              torch.nn.Linear(4, 2))
    for source in (net, list(net.named_parameters())):
        decay, no_decay = split_decay_groups(source, 5e-5)
        assert decay["weight_decay"] == 5e-5
        assert no_decay["weight_decay"] == 0.0
        # order is that of named_parameters() within each group
        assert [id(p) for p in decay["params"]] == \
            [id(net[0].weight), id(net[2].weight)]
        assert [id(p) for p in no_decay["params"]] == \
            [id(net[0].bias), id(net[1].weight), id(net[1].bias),
             id(net[2].bias)]
        both = decay["params"] + no_decay["params"]
        assert sorted(map(id, both)) == sorted(map(id, net.parameters()))
        assert len(set(map(id, both))) == len(both) == 6
    # a shared parameter is taken once
    named = list(net.named_parameters())
    decay, no_decay = split_decay_groups(named + named[:1], 0.1)
    assert len(decay["params"]) == 2 and len(no_decay["params"]) == 4
    # the groups are what the optimizers take
    opt = FusedLARS(split_decay_groups(net, 5e-5), lr=0.1)
    assert [g["weight_decay"] for g in opt.param_groups] == [5e-5, 0.0]
    assert all(g["trust_coefficient"] == 0.001 for g in opt.param_groups)


DISTRIBUTED_BODY = """
        import warnings
        from horovod_amd.ops import FusedLARS
        warnings.simplefilter("ignore")
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
        scales = [0.02, 0.3, 3.0, 10.0, 1.0]
        kw = dict(lr=0.5, momentum=0.8, weight_decay=0.02,
                  trust_coefficient=0.03, eps=1e-6, nesterov=True,
                  trust_clip=True, always_adapt=True, max_grad_norm=1.0)

        def params(seed):
            g = torch.Generator().manual_seed(seed)
            return [(torch.randn(s, generator=g) * sc).requires_grad_(True)
                    for s, sc in zip(shapes, scales)]

        def grads(step):
            g = torch.Generator().manual_seed(100 + step)
            return [torch.randn(s, generator=g) for s in shapes]

        ps_w, ps_u = params(5), params(5)
        wrapped = hvd.DistributedOptimizer(FusedLARS(ps_w, **kw))
        plain = FusedLARS(ps_u, **kw)
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


def test_distributed_optimizer_keeps_lars_options():
    """DistributedOptimizer rebuilds the optimizer from param_groups: every
    option, set to a non-default value here, must survive that, and the
    trajectory must be bitwise the unwrapped one.  Runs in a worker process
    so no initialised core outlives the test."""
    run_workers(1, DISTRIBUTED_BODY, timeout=120)
