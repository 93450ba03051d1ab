"""Loss scaling in FusedSGD, FusedAdamW and FusedLAMB: the native surface
exists after build(), and the semantics hold on CPU parameters through the
eager update (no GPU needed).

The oracle is the plain path: for a power-of-two scale S the scaled
optimizer, fed S * g, must equal the unscaled optimizer fed g bit for bit,
because (S * g) * (1 / S) is g exactly.  Gradients are made in the
parameter's dtype first and then multiplied by the current scale (2**8 ..
2**10 here, |g| < 8, so fp16 stays finite).  Inputs are those of
test_master_weights_build.py.
"""
import copy
import warnings

import pytest
import torch

from tests.parallel_util import run_workers
from tests.test_master_weights_build import (ADAMW_KW, STATE_KEYS, _grads,
                                             _make, _params)

NAMES = ["FusedSGD", "FusedAdamW", "FusedLAMB"]
# dtype of the parameters, and whether they get fp32 masters
FORMS = {"fp32": (torch.float32, False), "fp16": (torch.float16, True),
         "bf16": (torch.bfloat16, True)}
S = 2.0 ** 8
DYNAMIC = dict(loss_scale="dynamic", loss_scale_args=dict(
    init_scale=S, growth_interval=2))


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same_state(a, ps, b, qs):
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), i
        sa, sb = a.state[p], b.state[q]
        assert set(sa) == set(sb)
        for key in sa:
            if key in STATE_KEYS:
                assert torch.equal(_bits(sa[key]), _bits(sb[key])), (i, key)
            else:
                assert int(sa[key]) == int(sb[key]), (i, key)


# ---- the options and the native surface -------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_options_are_kept_in_param_groups(name):
    import horovod_amd.ops as ops
    cls = getattr(ops, name)
    p = [torch.zeros(3, requires_grad=True)]
    opt = cls(p, **DYNAMIC)
    assert opt.param_groups[0]["loss_scale"] == "dynamic"
    assert opt.param_groups[0]["loss_scale_args"] == DYNAMIC["loss_scale_args"]
    assert cls(p, loss_scale=128).param_groups[0]["loss_scale"] == 128
    plain = cls(p)
    assert plain.param_groups[0]["loss_scale"] is None
    assert plain.param_groups[0]["loss_scale_args"] is None
    assert plain.loss_scale_tensor is None and plain.get_loss_scale() is None
    assert "loss_scaler" not in plain.state_dict()
    assert cls._GROUP_DEFAULTS["loss_scale"] is None
    assert cls._GROUP_DEFAULTS["loss_scale_args"] is None
    assert cls._step_supports_amp_scaling is True
    # the defaults of dynamic scaling
    assert cls(p, loss_scale="dynamic").get_loss_scale() == 2.0 ** 16
    # a foreign state dict knows nothing of the options
    sd = opt.state_dict()
    del sd["param_groups"][0]["loss_scale"]
    del sd["param_groups"][0]["loss_scale_args"]
    del sd["loss_scaler"]
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["loss_scale"] is None


@pytest.mark.parametrize("bad", [
    dict(loss_scale=0), dict(loss_scale=-2.0), dict(loss_scale="static"),
    dict(loss_scale=float("inf")), dict(loss_scale=True),
    dict(loss_scale_args=dict(init_scale=4.0)),                # no loss_scale
    dict(loss_scale=4.0, loss_scale_args=dict(init_scale=4.0)),
    dict(loss_scale="dynamic", loss_scale_args=dict(scale=4.0)),
    dict(loss_scale="dynamic", loss_scale_args=dict(init_scale=0.0)),
    dict(loss_scale="dynamic", loss_scale_args=dict(growth_factor=0.5)),
    dict(loss_scale="dynamic", loss_scale_args=dict(backoff_factor=2.0)),
    dict(loss_scale="dynamic", loss_scale_args=dict(growth_interval=0)),
    dict(loss_scale="dynamic", loss_scale_args=dict(growth_interval=1.5)),
], ids=str)
def test_bad_values_are_rejected(bad):
    from horovod_amd.ops import FusedAdamW, FusedLAMB, FusedSGD
    p = [torch.zeros(3, requires_grad=True)]
    for cls in (FusedSGD, FusedAdamW, FusedLAMB):
        with pytest.raises(ValueError, match="loss_scale"):
            cls(p, **bad)
        with pytest.raises(ValueError, match="loss_scale"):
            cls([dict(params=p, **bad)])
        # set through a param-group dict later: at step()
        opt = cls(p, **DYNAMIC)
        opt.param_groups[0].update(
            dict(dict(loss_scale=None, loss_scale_args=None), **bad))
        p[0].grad = torch.ones(3)
        with pytest.raises(ValueError, match="loss_scale"):
            opt.step()


@pytest.mark.parametrize("name", NAMES)
def test_differing_group_values_raise_at_step(name):
    import horovod_amd.ops as ops
    a = torch.zeros(3, requires_grad=True)
    b = torch.zeros(3, requires_grad=True)
    a.grad, b.grad = torch.ones(3), torch.ones(3)
    for other in (dict(), dict(loss_scale=2.0),
                  dict(loss_scale="dynamic",
                       loss_scale_args=dict(init_scale=2.0))):
        opt = getattr(ops, name)([dict(params=[a], **DYNAMIC),
                                  dict(params=[b], **other)], lr=0.1)
        with pytest.raises(ValueError, match="every param group"):
            opt.step()
    assert torch.equal(a, torch.zeros(3)) and torch.equal(b, torch.zeros(3))


def test_core_steps_take_skip():
    from horovod_amd import _core
    calls = {
        "fused_sgd_step": lambda t, s: _core.fused_sgd_step(
            [t[0]], [t[1]], [t[2]], 0.1, 0.9, 0.01, 0.0, False, skip=s),
        "fused_adamw_step": lambda t, s: _core.fused_adamw_step(
            [t[0]], [t[1]], [t[2]], [t[3]], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1,
            skip=s),
        "fused_lamb_step": lambda t, s: _core.fused_lamb_step(
            [t[0]], [t[1]], [t[2]], [t[3]], 1e-3, 0.9, 0.999, 1e-6, 0.01, 1,
            True, True, skip=s),
    }
    for name, call in calls.items():
        assert "skip" in getattr(_core, name).__doc__, name
        # validation comes before any launch: CPU tensors are an error, not
        # a quiet fallback, and nothing is touched
        t = [torch.ones(4) for _ in range(4)]
        with pytest.raises(RuntimeError, match="GPU"):
            call(t, torch.zeros(1))
        with pytest.raises(RuntimeError, match="GPU"):
            call(t, None)
        assert all(torch.equal(x, torch.ones(4)) for x in t)


def test_core_scaled_norm_surface():
    from horovod_amd import _core
    doc = _core.multi_tensor_scaled_grad_norm.__doc__
    for word in ("grads", "max_norm", "scale", "found_inf", "growth_tracker",
                 "growth_factor", "backoff_factor", "growth_interval"):
        assert word in doc, word
    g, scale = [torch.ones(4)], torch.full((), S)
    tracker = torch.zeros((), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.multi_tensor_scaled_grad_norm(g, 1.0, scale, None, tracker,
                                            2.0, 0.5, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.multi_tensor_scaled_grad_norm(g)
    assert scale.item() == S and tracker.item() == 0


def test_scaled_finalize_kernel_is_built():
    from horovod_amd import _core
    with open(_core.__file__, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    assert b"scaled_clip_finalize_k" in blob
    assert b"clip_finalize_k" in blob.replace(b"scaled_clip_finalize_k", b"")


# ---- semantics through the eager update -------------------------------------

def _run(name, form, extra, calls=6, bad_call=2, scales=None, **scaling):
    """`calls` steps of the scaled optimizer, an inf in call `bad_call`; the
    plain one gets the other gradient sets.  -> both and their parameters."""
    dtype, master = FORMS[form]
    ps, qs = _params(dtype), _params(dtype)
    extra = dict(extra, master_weights=master)
    scaled = _make(name, ps, **dict(scaling, **extra))
    plain = _make(name, qs, **extra)
    for call in range(calls):
        scale = scaled.get_loss_scale()
        if scales is not None:
            assert scale == scales[call], (call, scale)
        grads = _grads(call, dtype)
        for p, g in zip(ps, grads):
            p.grad = g * scale
            assert p.grad.dtype == dtype and torch.isfinite(p.grad).all()
        if call == bad_call:
            ps[1].grad[5, 5] = float("inf")
        fed = [p.grad.clone() for p in ps]
        before = [p.detach().clone() for p in ps]
        scaled.step()
        assert all(torch.equal(_bits(p.grad), _bits(g))
                   for p, g in zip(ps, fed)), "step() must not write p.grad"
        assert scaled.last_found_inf.item() == (call == bad_call)
        if call == bad_call:
            assert all(torch.equal(_bits(p.detach()), _bits(b))
                       for p, b in zip(ps, before))
            continue
        for q, g in zip(qs, grads):
            q.grad = g
        plain.step()
        assert not torch.equal(ps[0].detach(), before[0])
    return scaled, ps, plain, qs


@pytest.mark.parametrize("mode", ["static", "dynamic"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_scaled_eager_update_equals_plain_bitwise(name, form, mode):
    scaling = DYNAMIC if mode == "dynamic" else dict(loss_scale=S)
    scales = [S, S, 2 * S, S, S, 2 * S] if mode == "dynamic" else [S] * 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaled, ps, plain, qs = _run(name, form, {}, scales=scales, **scaling)
    _same_state(scaled, ps, plain, qs)
    assert scaled.skipped_steps == 1
    if name != "FusedSGD":
        assert all(int(scaled.state[p]["step"]) == 5 for p in ps)
    for p in ps:
        if FORMS[form][1]:
            assert torch.equal(
                p.detach(), scaled.state[p]["master_param"].to(p.dtype))


@pytest.mark.parametrize("name", NAMES)
def test_scaled_and_clipped_fp32_equals_plain_bitwise(name):
    """With max_grad_norm the coefficient is clip / S and last_grad_norm the
    unscaled norm."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaled, ps, plain, qs = _run(name, "fp32", dict(max_grad_norm=1.0),
                                     **DYNAMIC)
    _same_state(scaled, ps, plain, qs)
    assert torch.equal(scaled.last_grad_norm, plain.last_grad_norm)
    assert plain.last_grad_norm.item() > 10, "the clip is active"


def test_overflow_in_the_first_call_leaves_a_fresh_state():
    from horovod_amd.ops import FusedAdamW
    p = torch.ones(4, requires_grad=True)
    opt = FusedAdamW([p], **DYNAMIC)
    p.grad = torch.full((4,), float("nan"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step()
    st = opt.state[p]
    assert st["step"] == 0 and opt.skipped_steps == 1
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert torch.equal(p.detach(), torch.ones(4))
    assert opt.get_loss_scale() == S / 2


def test_scale_sequence_follows_torch_amp_update_scale():
    """The scale over a scripted run of overflows, growth_interval=2,
    against torch._amp_update_scale_."""
    from horovod_amd.ops import FusedSGD
    flags = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    p = torch.ones(4, requires_grad=True)
    opt = FusedSGD([p], lr=0.1, **DYNAMIC)
    ref_scale = torch.full((), S)
    ref_tracker = torch.zeros((), dtype=torch.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call, flag in enumerate(flags):
            p.grad = torch.full((4,), float("inf") if flag else 1.0)
            opt.step()
            torch._amp_update_scale_(ref_scale, ref_tracker,
                                     torch.full((), float(flag)), 2.0, 0.5, 2)
            sd = opt.state_dict()["loss_scaler"]
            assert sd == {"scale": ref_scale.item(),
                          "growth_tracker": ref_tracker.item()}, call
    assert opt.skipped_steps == sum(flags)
    # growth that would overflow keeps the scale
    opt = FusedSGD([p], lr=0.1, loss_scale="dynamic", loss_scale_args=dict(
        init_scale=2.0 ** 127, growth_interval=1))
    p.grad = torch.zeros(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step()
    assert opt.state_dict()["loss_scaler"] == {"scale": 2.0 ** 127,
                                               "growth_tracker": 0}


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_round_trip_restores_the_scaler(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaled, ps, _, _ = _run(name, "fp16", {}, calls=4, **DYNAMIC)
        sd = copy.deepcopy(scaled.state_dict())
        assert sd["loss_scaler"] == {"scale": S, "growth_tracker": 1}
        rs = [p.detach().clone().requires_grad_(True) for p in ps]
        loaded = _make(name, rs, master_weights=True, **DYNAMIC)
        assert loaded.get_loss_scale() == S
        loaded.load_state_dict(sd)
        assert loaded.state_dict()["loss_scaler"] == sd["loss_scaler"]
        # a dict without the entry loads and keeps what is there
        del sd["loss_scaler"]
        loaded.load_state_dict(sd)
        assert loaded.state_dict()["loss_scaler"] == {"scale": S,
                                                      "growth_tracker": 1}
        for call in range(4, 6):
            for a, b, g in zip(ps, rs, _grads(call, torch.float16)):
                a.grad = g * scaled.get_loss_scale()
                b.grad = g * loaded.get_loss_scale()
            scaled.step()
            loaded.step()
    assert scaled.get_loss_scale() == loaded.get_loss_scale() == 2 * S
    _same_state(scaled, ps, loaded, rs)


# ---- torch.amp.GradScaler ---------------------------------------------------

def _scaler():
    return torch.amp.GradScaler("cpu", init_scale=S, growth_interval=2)


def test_grad_scaler_steps_fp16_master_parameters_cpu():
    """GradScaler.step() refuses fp16 gradients ("Attempting to unscale FP16
    gradients") of an optimizer that does not unscale itself.  Here it hands
    scale and flag to step(): the parameters step, and an overflow skips."""
    from horovod_amd.ops import FusedAdamW
    ps, qs = _params(torch.float16), _params(torch.float16)
    sc = _scaler()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedAdamW(ps, master_weights=True, **ADAMW_KW)
        plain = FusedAdamW(qs, master_weights=True, **ADAMW_KW)
        for call in range(5):
            scale = sc.scale(torch.ones(())).item()
            assert scale == [S, S, 2 * S, S, S][call]
            grads = _grads(call, torch.float16)
            for p, g in zip(ps, grads):
                p.grad = g * scale
            if call == 2:
                ps[1].grad[0, 0] = float("inf")
            sc.step(opt)
            sc.update()
            assert not hasattr(opt, "grad_scale")
            if call != 2:
                for q, g in zip(qs, grads):
                    q.grad = g
                plain.step()
    assert opt.skipped_steps == 1
    assert all(opt.state[p]["step"] == 4 for p in ps)
    _same_state(opt, ps, plain, qs)


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
def test_grad_scaler_trajectory_matches_torch_adamw_cpu(clip):
    from horovod_amd.ops import FusedAdamW
    ps, qs = _params(torch.float32), _params(torch.float32)
    ref = torch.optim.AdamW(qs, **ADAMW_KW)
    sc, sc_ref = _scaler(), _scaler()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedAdamW(ps, max_grad_norm=clip, **ADAMW_KW)
        for call in range(5):
            scale = sc.scale(torch.ones(())).item()
            assert sc_ref.scale(torch.ones(())).item() == scale
            for p, q, g in zip(ps, qs, _grads(call, torch.float32)):
                p.grad = g * scale
                q.grad = g * scale
            if call == 2:
                ps[1].grad[0, 0] = float("inf")
                qs[1].grad[0, 0] = float("inf")
            if clip is not None:
                sc_ref.unscale_(ref)
                torch.nn.utils.clip_grad_norm_(qs, clip)
            sc.step(opt)
            sc_ref.step(ref)
            sc.update()
            sc_ref.update()
            for i, (p, q) in enumerate(zip(ps, qs)):
                assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), \
                    (call, i, (p - q).abs().max().item())
    assert sc.get_scale() == sc_ref.get_scale() == 2 * S
    assert opt.skipped_steps == 1
    assert not torch.equal(ps[0].detach(), _params(torch.float32)[0])


def test_grad_scaler_and_loss_scale_option_exclude_each_other():
    from horovod_amd.ops import FusedAdamW
    p = torch.ones(4, requires_grad=True)
    opt = FusedAdamW([p], **DYNAMIC)
    sc = _scaler()
    sc.scale(torch.ones(()))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="GradScaler"):
        sc.step(opt)
    assert torch.equal(p.detach(), torch.ones(4))


# ---- hvd.DistributedOptimizer and the broadcasts ----------------------------

TWO_RANK_BODY = """
        import warnings
        from horovod_amd.ops import FusedAdamW, FusedSGD
        warnings.simplefilter("ignore")
        shapes = [(33,), (128, 64), (7, 3, 3)]
        S = 2.0 ** 8
        scaling = dict(loss_scale="dynamic", loss_scale_args=dict(
            init_scale=S, growth_interval=2))

        def randn(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g) for s in shapes]

        def same_on_all_ranks(ts, name):
            mine = torch.cat([t.detach().reshape(-1) for t in ts])
            root = hvd.broadcast(mine.clone(), 0, name=name)
            assert torch.equal(mine.view(torch.int32), root.view(torch.int32))

        ps = [p.requires_grad_(True) for p in randn(1)]   # same on all ranks
        start = [p.detach().clone() for p in ps]
        opt = hvd.DistributedOptimizer(
            FusedAdamW(ps, lr=1e-2, max_grad_norm=1.0, **scaling),
            named_parameters=[(f"p{i}", p) for i, p in enumerate(ps)])
        for group in opt.param_groups:
            assert group["loss_scale"] == "dynamic"
            assert group["loss_scale_args"] == scaling["loss_scale_args"]
        # only rank 1 overflows: the flag comes from the reduced gradients
        for p, g in zip(ps, randn(50 + rank)):
            p.grad = g * opt.get_loss_scale()
        if rank == 1:
            ps[1].grad[3, 3] = float("inf")
        opt.step()
        assert opt.last_found_inf.item() == 1.0
        assert opt.get_loss_scale() == S / 2 and opt.skipped_steps == 1
        for p, p0 in zip(ps, start):
            assert torch.equal(p.detach(), p0)
            assert opt.state[p]["step"] == 0
        # a clean step on the halved scale, the same everywhere
        for p, g in zip(ps, randn(60 + rank)):
            p.grad = g * opt.get_loss_scale()
        opt.step()
        assert opt.get_loss_scale() == S / 2 and opt.skipped_steps == 1
        assert all(opt.state[p]["step"] == 1 for p in ps)
        assert not torch.equal(ps[0].detach(), start[0])
        same_on_all_ranks(ps, "ls.params")

        # every rank arrives with a scaler of its own; root's is carried
        for cls, kw in ((FusedAdamW, {}), (FusedSGD, {})):
            qs = [p.requires_grad_(True) for p in randn(2)]
            mine = cls(qs, lr=1e-2, **dict(scaling, **kw))
            for step in range(1 + rank):
                for q, g in zip(qs, randn(70 + step)):
                    q.grad = g * float("inf")
                mine.step()
            assert mine.get_loss_scale() == S / 2 ** (1 + rank)
            wrapped = hvd.DistributedOptimizer(cls(qs, lr=1e-2, **dict(
                scaling, **kw)))
            assert wrapped.get_loss_scale() == S, "rebuilt: starts afresh"
            wrapped.load_state_dict(mine.state_dict())
            assert wrapped.get_loss_scale() == S / 2 ** (1 + rank)
            hvd.broadcast_optimizer_state(wrapped, root_rank=0)
            assert wrapped.state_dict()["loss_scaler"] == {
                "scale": S / 2, "growth_tracker": 0}, cls
"""


def test_two_ranks_one_overflows_both_skip():
    """Through hvd.DistributedOptimizer with no manual synchronize, one
    rank's inf skips the step and halves the scale on both ranks; and
    broadcast_optimizer_state carries root's scale and tracker."""
    run_workers(2, TWO_RANK_BODY, timeout=240)
