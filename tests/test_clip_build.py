"""Global-norm clipping in FusedSGD / FusedAdamW: the native surface exists
after build() and the option works on CPU parameters through the torch-op
path (no GPU needed)."""
import copy

import pytest
import torch

from tests.parallel_util import run_workers

SHAPES = [(33,), (128, 64), (7, 3, 3), (1024,)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]
    return ps, [p.detach().clone().requires_grad_(True) for p in ps]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) for s in SHAPES]


def _run(opt_f, ps_f, opt_r, ps_r, rtol, atol, steps=6):
    """Clipped fused optimizer vs clip_grad_norm_ + the torch optimizer."""
    for step in range(steps):
        grads = _grads(step)
        for p, q, g in zip(ps_f, ps_r, grads):
            p.grad = g.clone()
            q.grad = g.clone()
        opt_f.step()
        norm = torch.nn.utils.clip_grad_norm_(ps_r, 1.0)
        opt_r.step()
        assert norm > 90, norm        # ~96: the clip is active
        assert torch.equal(opt_f.last_grad_norm, norm), \
            (opt_f.last_grad_norm, norm)
        assert opt_f.last_grad_norm.dim() == 0
        for p, g in zip(ps_f, grads):
            assert torch.equal(p.grad, g), "step() must not scale p.grad"
        for i, (p, q) in enumerate(zip(ps_f, ps_r)):
            assert torch.allclose(p, q, rtol=rtol, atol=atol), \
                (step, i, (p - q).abs().max().item())


def test_core_exports_clip_symbols():
    from horovod_amd import _core
    for name in ("multi_tensor_grad_norm", "multi_tensor_scale_"):
        assert callable(getattr(_core, name, None)), name


def test_fused_adamw_clip_matches_torch_cpu():
    from horovod_amd.ops import FusedAdamW
    ps_f, ps_r = _params(5)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    with pytest.warns(UserWarning, match="eager"):
        _run(FusedAdamW(ps_f, max_grad_norm=1.0, **kw), ps_f,
             torch.optim.AdamW(ps_r, **kw), ps_r, rtol=1e-5, atol=1e-6)


def test_fused_sgd_clip_matches_torch_cpu():
    from horovod_amd.ops import FusedSGD
    ps_f, ps_r = _params(9)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01)
    with pytest.warns(UserWarning, match="eager"):
        _run(FusedSGD(ps_f, max_grad_norm=1.0, **kw), ps_f,
             torch.optim.SGD(ps_r, **kw), ps_r, rtol=1e-5, atol=1e-6)


def test_fused_adamw_continues_torch_adamw_state_dict_cpu():
    """torch.optim.AdamW keeps `step` as a tensor; FusedAdamW loads that
    state dict and follows torch from there."""
    from horovod_amd.ops import FusedAdamW
    ps_f, ps_r = _params(5)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    ref = torch.optim.AdamW(ps_r, **kw)
    for step in range(2):
        for q, g in zip(ps_r, _grads(step)):
            q.grad = g.clone()
        ref.step()
    assert torch.is_tensor(ref.state[ps_r[0]]["step"])
    for p, q in zip(ps_f, ps_r):
        p.data.copy_(q.data)
    opt = FusedAdamW(ps_f, **kw)
    # a copy, as if saved and loaded: load_state_dict keeps the step tensor
    # it is given, and ref goes on counting in its own
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert torch.is_tensor(opt.state[ps_f[0]]["step"])
    with pytest.warns(UserWarning, match="eager"):
        for step in range(2, 5):
            for p, q, g in zip(ps_f, ps_r, _grads(step)):
                p.grad = g.clone()
                q.grad = g.clone()
            opt.step()
            ref.step()
            for i, (p, q) in enumerate(zip(ps_f, ps_r)):
                assert int(opt.state[p]["step"]) == step + 1
                assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), \
                    (step, i, (p - q).abs().max().item())


@pytest.mark.parametrize("kw", [dict(lr=0.1),
                                dict(lr=0.1, momentum=0.9, weight_decay=0.01),
                                dict(lr=0.1, momentum=0.9, nesterov=True)],
                         ids=["plain", "momentum_wd", "nesterov"])
def test_fused_sgd_sparse_gradient_matches_torch_on_dense(kw):
    """A sparse gradient takes the eager update on its densified value."""
    from horovod_amd.ops import FusedSGD
    g = torch.Generator().manual_seed(3)
    p = torch.randn(50, 8, generator=g).requires_grad_(True)
    q = p.detach().clone().requires_grad_(True)
    opt, ref = FusedSGD([p], **kw), torch.optim.SGD([q], **kw)
    with pytest.warns(UserWarning, match="FusedSGD.*eager"):
        for step in range(3):
            rows = torch.randperm(50, generator=g)[:7]
            values = torch.randn(7, 8, generator=g)
            sparse = torch.sparse_coo_tensor(rows.unsqueeze(0), values,
                                             (50, 8))
            p.grad = sparse
            q.grad = sparse.to_dense()
            opt.step()
            ref.step()
            assert p.grad.is_sparse, "step() must not replace p.grad"
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), \
                (step, (p - q).abs().max().item())
    assert not torch.equal(p.detach(), torch.zeros_like(p))


DISTRIBUTED_BODY = """
        import warnings
        from horovod_amd.ops import FusedAdamW, FusedSGD
        warnings.simplefilter("ignore")
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,)]

        def params(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).requires_grad_(True)
                    for s in shapes]

        def grads(step):
            g = torch.Generator().manual_seed(100 + step)
            return [torch.randn(s, generator=g) for s in shapes]

        # AdamW: the option survives the rebuild from param_groups and the
        # trajectory is the unwrapped one
        ps_w, ps_u = params(5), params(5)
        wrapped = hvd.DistributedOptimizer(
            FusedAdamW(ps_w, lr=1e-2, max_grad_norm=1.0))
        plain = FusedAdamW(ps_u, lr=1e-2, max_grad_norm=1.0)
        assert all(g["max_grad_norm"] == 1.0 for g in wrapped.param_groups)
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

        # AdamW barely depends on the gradient's scale, so show on plain SGD
        # that the wrapped optimizer really clips: p -= lr * g / norm
        a, b = params(7), params(7)
        oa = hvd.DistributedOptimizer(FusedSGD(a, lr=0.1, max_grad_norm=1.0))
        for p, g in zip(a, grads(0)):
            p.grad = g.clone()
        oa.step()
        total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads(0)))
        for p, p0, g in zip(a, b, grads(0)):
            want = p0.detach() - 0.1 * g * float(1.0 / (total + 1e-6))
            assert torch.allclose(p.detach(), want, rtol=1e-5, atol=1e-6)
"""


def test_distributed_optimizer_keeps_max_grad_norm():
    """DistributedOptimizer rebuilds the optimizer from param_groups; after
    hvd.init() in a single process the option must survive that, the
    trajectory must equal the unwrapped one and the clip must be applied.
    Runs in a worker process so no initialised core outlives the test."""
    run_workers(1, DISTRIBUTED_BODY, timeout=120)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0])
def test_non_positive_max_grad_norm_raises(bad):
    from horovod_amd.ops import FusedAdamW, FusedSGD
    p = [torch.zeros(3, requires_grad=True)]
    with pytest.raises(ValueError):
        FusedAdamW(p, max_grad_norm=bad)
    with pytest.raises(ValueError):
        FusedSGD(p, max_grad_norm=bad)
    # given through a param-group dict, at construction or later
    for cls in (FusedAdamW, FusedSGD):
        with pytest.raises(ValueError):
            cls([{"params": p, "max_grad_norm": bad}])
        opt = cls(p, max_grad_norm=1.0)
        opt.param_groups[0]["max_grad_norm"] = bad
        p[0].grad = torch.ones(3)
        with pytest.raises(ValueError):
            opt.step()


def test_differing_group_values_raise_at_step():
    from horovod_amd.ops import FusedAdamW, FusedSGD
    for cls in (FusedAdamW, FusedSGD):
        a = torch.zeros(3, requires_grad=True)
        b = torch.zeros(3, requires_grad=True)
        opt = cls([{"params": [a], "max_grad_norm": 1.0},
                   {"params": [b], "max_grad_norm": 2.0}], lr=0.1)
        a.grad = torch.ones(3)
        b.grad = torch.ones(3)
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.step()
        opt = cls([{"params": [a], "max_grad_norm": 1.0},
                   {"params": [b]}], lr=0.1)
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.step()


def test_functional_clip_defers_to_torch_on_cpu():
    from horovod_amd.ops import clip_grad_norm_
    ps, qs = _params(3)
    for p, q, g in zip(ps, qs, _grads(0)):
        p.grad = g.clone()
        q.grad = g.clone()
    n1 = clip_grad_norm_(ps, 1.0)
    n2 = torch.nn.utils.clip_grad_norm_(qs, 1.0)
    assert torch.equal(n1, n2)
    for p, q in zip(ps, qs):
        assert torch.equal(p.grad, q.grad)
