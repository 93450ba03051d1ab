"""master_weights=True on FusedSGD, FusedAdamW and FusedLAMB: the native
surface exists after build(), and the semantics hold on CPU fp16/bf16
parameters through the eager master-weight update (no GPU needed).

The reference is the fp64 evaluation of each definition (RefLamb of
test_lamb_build.py, adamw_definition and sgd_definition of
test_gpu_fused_steps.py), started from the rounded parameters and fed the
gradients rounded to the parameter's dtype, as the optimizer sees them.  The
fp32 `master_param` is held to it at the project's rtol=1e-5, atol=1e-6.

Inputs are those of test_lamb_build.py.  Measured on the CPU before they
were fixed: over 6 steps an fp32 torch evaluation of the same formulas uses
at most 0.24 of that bound for the SGD variants (lr=0.1, momentum 0.9), 0.05
for AdamW and 0.10 for LAMB (worst |err| / (atol + rtol * |ref|) over all
tensors, steps and both dtypes), so under one half everywhere.
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers
from tests.test_gpu_fused_steps import adamw_definition, sgd_definition
from tests.test_lamb_build import (ATOL, KW, RTOL, SCALES, SHAPES, STEPS,
                                   RefLamb)

LOW = {"fp16": torch.float16, "bf16": torch.bfloat16}
SGD_KW = {
    "plain": dict(lr=0.1, momentum=0.0, weight_decay=0.01, dampening=0.0,
                  nesterov=False),
    "momentum": dict(lr=0.1, momentum=0.9, weight_decay=0.01, dampening=0.0,
                     nesterov=False),
    "nesterov": dict(lr=0.1, momentum=0.9, weight_decay=0.01, dampening=0.0,
                     nesterov=True),
}
ADAMW_KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
STATE_KEYS = ("master_param", "exp_avg", "exp_avg_sq", "momentum_buffer")


def _params(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * sc).to(dtype).requires_grad_(True)
            for s, sc in zip(SHAPES, SCALES)]


def _grads(step, dtype):
    """Rounded to the parameter's dtype, as backward would hand them over."""
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g).to(dtype) for s in SHAPES]


def _feed(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()


def _make(name, ps, **extra):
    import horovod_amd.ops as ops
    kw = {"FusedSGD": SGD_KW["nesterov"], "FusedAdamW": ADAMW_KW,
          "FusedLAMB": KW}[name]
    return getattr(ops, name)(ps, **dict(kw, **extra))


# ---- the definitions, iterated in the dtype `acc` ---------------------------

class RefSgd:
    def __init__(self, params, kw, acc=torch.float64):
        self.acc, self.kw = acc, kw
        self.p = [p.detach().to(acc) for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]

    def step(self, grads):
        for i, g in enumerate(grads):
            self.p[i], self.m[i] = sgd_definition(
                [self.p[i], g.to(self.acc), self.m[i]], 1.0, **self.kw)


class RefAdamw:
    def __init__(self, params, acc=torch.float64):
        self.acc, self.t = acc, 0
        self.p = [p.detach().to(acc) for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]

    def step(self, grads):
        self.t += 1
        b1, b2 = ADAMW_KW["betas"]
        for i, g in enumerate(grads):
            self.p[i], self.m[i], self.v[i] = adamw_definition(
                [self.p[i], g.to(self.acc), self.m[i], self.v[i]], 1.0,
                self.t, ADAMW_KW["lr"], b1, b2, ADAMW_KW["eps"],
                ADAMW_KW["weight_decay"])


def _reference(name, ps, sgd_kw=None):
    if name == "FusedSGD":
        return RefSgd(ps, sgd_kw)
    if name == "FusedAdamW":
        return RefAdamw(ps)
    return RefLamb([p.detach().float() for p in ps], **KW)


def _used(got, want):
    """Share of the bound that `got` uses against the fp64 `want`."""
    err = (got.double() - want).abs()
    return (err / (ATOL + RTOL * want.abs())).max().item()


# ---- the option and the native surface --------------------------------------

@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdamW", "FusedLAMB"])
def test_option_is_accepted_and_kept_in_param_groups(name):
    import horovod_amd.ops as ops
    p = [torch.zeros(3, requires_grad=True)]
    opt = getattr(ops, name)(p, master_weights=True)
    assert opt.param_groups[0]["master_weights"] is True
    assert getattr(ops, name)(p).param_groups[0]["master_weights"] is False
    assert opt._GROUP_DEFAULTS["master_weights"] is False
    # a foreign state dict knows nothing of the option
    sd = opt.state_dict()
    del sd["param_groups"][0]["master_weights"]
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["master_weights"] is False


def test_core_steps_take_model_params():
    from horovod_amd import _core
    calls = {
        "fused_sgd_step": lambda t, q: _core.fused_sgd_step(
            [t[0]], [t[1]], [t[2]], 0.1, 0.9, 0.01, 0.0, False,
            model_params=q),
        "fused_adamw_step": lambda t, q: _core.fused_adamw_step(
            [t[0]], [t[1]], [t[2]], [t[3]], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1,
            model_params=q),
        "fused_lamb_step": lambda t, q: _core.fused_lamb_step(
            [t[0]], [t[1]], [t[2]], [t[3]], 1e-3, 0.9, 0.999, 1e-6, 0.01, 1,
            True, True, model_params=q),
    }
    for name, call in calls.items():
        assert "model_params" in getattr(_core, name).__doc__, name
        # validation comes before any launch: CPU tensors are an error, not
        # a quiet fallback, and nothing is touched
        t = [torch.ones(4), torch.ones(4).bfloat16(), torch.ones(4),
             torch.ones(4)]
        q = torch.full((4,), 3.0).bfloat16()
        with pytest.raises(RuntimeError, match="GPU"):
            call(t, [q])
        with pytest.raises(RuntimeError, match="as many model_params"):
            call(t, [])
        assert torch.equal(t[0], torch.ones(4))
        assert torch.equal(q, torch.full((4,), 3.0).bfloat16())


def test_master_weight_kernels_are_built():
    """Every optimizer kernel is instantiated for __half and __hip_bfloat16
    next to the fp32 one, in the gfx950 build."""
    from horovod_amd import _core
    with open(_core.__file__, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for kernel in (b"fused_sgd_k", b"fused_adamw_k", b"lamb_moments_k",
                   b"lamb_update_k"):
        for lp in (b"Iv", b"I6__half", b"I14__hip_bfloat16"):
            assert kernel + lp in blob, (kernel, lp)


# ---- semantics through the eager update -------------------------------------

def _run(name, low, steps=STEPS, sgd_variant="nesterov", check=True, **extra):
    dtype = LOW[low]
    ps = _params(dtype)
    if name == "FusedSGD":
        extra = dict(SGD_KW[sgd_variant], **extra)
    ref = _reference(name, ps, SGD_KW[sgd_variant])
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = _make(name, ps, master_weights=True, **extra)
        for step in range(steps):
            grads = _grads(step, dtype)
            _feed(ps, grads)
            opt.step()
            ref.step(grads)
            for i, (p, g, want) in enumerate(zip(ps, grads, ref.p)):
                st = opt.state[p]
                assert torch.equal(p.grad, g), "step() must not write p.grad"
                for key in STATE_KEYS:
                    if key in st:
                        assert st[key].dtype == torch.float32, key
                        assert st[key].shape == p.shape
                master = st["master_param"]
                assert p.dtype == dtype
                assert torch.equal(p.detach(), master.to(dtype)), (step, i)
                if check:
                    worst = max(worst, _used(master, want))
                    assert torch.allclose(master.double(), want, rtol=RTOL,
                                          atol=ATOL), \
                        (step, i, (master.double() - want).abs().max().item())
    return opt, ps, ref, worst


@pytest.mark.parametrize("low", list(LOW))
@pytest.mark.parametrize("variant", list(SGD_KW))
def test_sgd_master_follows_fp64_cpu(variant, low):
    opt, ps, _, _ = _run("FusedSGD", low, sgd_variant=variant)
    has_buffer = ["momentum_buffer" in opt.state[p] for p in ps]
    assert all(has_buffer) == (variant != "plain") and \
        any(has_buffer) == (variant != "plain")


@pytest.mark.parametrize("low", list(LOW))
def test_adamw_master_follows_fp64_cpu(low):
    opt, ps, _, _ = _run("FusedAdamW", low)
    assert set(opt.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq",
                                     "master_param"}


@pytest.mark.parametrize("low", list(LOW))
def test_lamb_master_follows_fp64_cpu(low):
    _, _, ref, _ = _run("FusedLAMB", low)
    # the inputs must make a wrong or missing trust ratio visible
    assert min(ref.trust) < 0.1 and max(ref.trust) > 5, ref.trust


def test_eager_master_update_warns_once():
    ps = _params(torch.bfloat16)
    opt = _make("FusedAdamW", ps, master_weights=True)
    _feed(ps, _grads(0, torch.bfloat16))
    with pytest.warns(UserWarning, match="FusedAdamW.*eager"):
        opt.step()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt.step()


def test_small_updates_are_kept_and_exp_avg_sq_decays():
    """What bf16 state loses: an update below 2^-9 of the weight, and the
    decay of exp_avg_sq by beta2 = 0.999."""
    from horovod_amd.ops import FusedAdamW, FusedSGD
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = torch.ones(8).bfloat16().requires_grad_(True)
        opt = FusedSGD([p], lr=2.0 ** -12, master_weights=True)
        for _ in range(16):
            p.grad = torch.ones(8).bfloat16()
            opt.step()
        assert torch.equal(opt.state[p]["master_param"],
                           torch.full((8,), 1 - 2.0 ** -8))
        assert torch.equal(p.detach(),
                           torch.full((8,), 1 - 2.0 ** -8).bfloat16())
        q = torch.ones(8).bfloat16().requires_grad_(True)
        opt = FusedAdamW([q], master_weights=True)
        q.grad = torch.ones(8).bfloat16()
        opt.step()
        first = opt.state[q]["exp_avg_sq"].clone()
        q.grad = torch.zeros(8).bfloat16()
        opt.step()
        assert torch.equal(opt.state[q]["exp_avg_sq"], first * 0.999)
        assert (opt.state[q]["exp_avg_sq"] < first).all()


@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdamW", "FusedLAMB"])
def test_default_keeps_low_precision_state(name):
    """master_weights=False: a bf16 parameter keeps bf16 moments and gets no
    master, as before."""
    ps = _params(torch.bfloat16)
    with pytest.warns(UserWarning, match="eager"):
        opt = _make(name, ps)
        _feed(ps, _grads(0, torch.bfloat16))
        opt.step()
    for p in ps:
        st = opt.state[p]
        assert "master_param" not in st
        moments = [st[k] for k in STATE_KEYS[1:] if k in st]
        assert moments and all(m.dtype == torch.bfloat16 for m in moments)


@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdamW", "FusedLAMB"])
def test_fp32_parameters_of_a_master_group_get_no_master(name):
    ps = _params(torch.bfloat16)
    fp32 = [p.detach().float().requires_grad_(True) for p in ps[:2]]
    alone = [p.detach().clone().requires_grad_(True) for p in fp32]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = _make(name, fp32 + ps, master_weights=True)
        ref = _make(name, alone)
        for step in range(2):
            grads = _grads(step, torch.bfloat16)
            _feed(ps, grads)
            _feed(fp32, [g.float() for g in grads[:2]])
            _feed(alone, [g.float() for g in grads[:2]])
            opt.step()
            ref.step()
    for p, q in zip(fp32, alone):
        assert "master_param" not in opt.state[p]
        assert torch.equal(p, q), "fp32 parameters are updated as ever"
    for p in ps:
        assert opt.state[p]["master_param"].dtype == torch.float32


# ---- state dict -------------------------------------------------------------

@pytest.mark.parametrize("low", list(LOW))
@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdamW", "FusedLAMB"])
def test_state_dict_round_trip_is_bitwise(name, low):
    import copy
    dtype = LOW[low]
    opt, ps, _, _ = _run(name, low, steps=3, check=False)
    sd = copy.deepcopy(opt.state_dict())
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded = _make(name, qs, master_weights=True)
        loaded.load_state_dict(sd)
        for p, q in zip(ps, qs):
            a, b = opt.state[p], loaded.state[q]
            assert set(a) == set(b)
            for key in STATE_KEYS:
                if key in a:
                    assert b[key].dtype == torch.float32, key
                    assert torch.equal(a[key], b[key]), key
                    assert b[key].data_ptr() != a[key].data_ptr()
            # what the loaded optimizer holds is not the dict's own tensor
            for st in sd["state"].values():
                assert all(b["master_param"].data_ptr() != t.data_ptr()
                           for t in st.values() if torch.is_tensor(t))
        for step in range(3, 6):
            grads = _grads(step, dtype)
            _feed(ps, grads)
            _feed(qs, grads)
            opt.step()
            loaded.step()
            for p, q in zip(ps, qs):
                assert torch.equal(p, q), step
                for key in STATE_KEYS:
                    if key in opt.state[p]:
                        assert torch.equal(opt.state[p][key],
                                           loaded.state[q][key]), (step, key)


# ---- hvd.DistributedOptimizer and the broadcasts ----------------------------

BROADCAST_BODY = """
        import warnings
        from horovod_amd.ops import FusedAdamW, FusedLAMB, FusedSGD
        warnings.simplefilter("ignore")
        shapes = [(33,), (128, 64), (7, 3, 3)]

        def params(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).bfloat16().requires_grad_(True)
                    for s in shapes]

        def grads(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).bfloat16() for s in shapes]

        for cls, kw in ((FusedSGD, dict(momentum=0.9)), (FusedAdamW, {}),
                        (FusedLAMB, {})):
            # every rank starts elsewhere and has taken its own steps
            ps = params(10 + rank)
            opt = hvd.DistributedOptimizer(
                cls(ps, lr=1e-2, master_weights=True, max_grad_norm=2.0,
                    **kw))
            for group in opt.param_groups:
                assert group["master_weights"] is True
                assert group["max_grad_norm"] == 2.0
            plain = cls(ps, lr=1e-2, master_weights=True, **kw)
            for step in range(2 + rank):
                for p, g in zip(ps, grads(50 + 7 * rank + step)):
                    p.grad = g
                plain.step()
            opt.load_state_dict(plain.state_dict())
            mine = [opt.state[p]["master_param"].clone() for p in ps]
            hvd.broadcast_parameters(ps, root_rank=0)
            hvd.broadcast_optimizer_state(opt, root_rank=0)
            keys = [k for k in ("master_param", "exp_avg", "exp_avg_sq",
                                "momentum_buffer") if k in opt.state[ps[0]]]
            assert len(keys) >= 2, keys
            for i, p in enumerate(ps):
                st = opt.state[p]
                for key in keys:
                    assert st[key].dtype == torch.float32, (key, st[key].dtype)
                    root = hvd.broadcast(st[key].clone(), 0,
                                         name=f"check.{cls.__name__}.{i}.{key}")
                    assert torch.equal(st[key].view(torch.int32),
                                       root.view(torch.int32)), (i, key)
                assert torch.equal(p.detach(),
                                   st["master_param"].bfloat16()), i
                same = torch.equal(st["master_param"], mine[i])
                assert same == (rank == 0), "root's masters, on every rank"
                if "step" in st:
                    assert int(st["step"]) == 2
            # and the next step is the same everywhere
            for p, g in zip(ps, grads(99)):
                p.grad = g
            opt.step()
            for i, p in enumerate(ps):
                m = opt.state[p]["master_param"]
                root = hvd.broadcast(m.clone(), 0,
                                     name=f"after.{cls.__name__}.{i}")
                assert torch.equal(m, root)
                assert torch.equal(p.detach(), m.bfloat16())
"""


def test_two_ranks_broadcast_roots_masters():
    """DistributedOptimizer keeps the option; after broadcast_parameters and
    broadcast_optimizer_state every rank holds root's fp32 masters bit for
    bit, and the parameter is the rounded master."""
    run_workers(2, BROADCAST_BODY, timeout=240)
