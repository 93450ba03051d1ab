"""Loss scaling on one MI355X: the `skip` flag of the step kernels, the
scaled norm pass (csrc/clip_kernels.hip, scaled_clip_finalize_k) and the
loss_scale option of FusedSGD / FusedAdamW / FusedLAMB.

The oracle of the optimizer tests is the plain path: for a power-of-two scale
S the scaled optimizer, fed S * g, must equal the unscaled optimizer fed g
bit for bit -- parameters, masters, moments, `step` and `last_grad_norm` --
because (S * g) * (c / S) rounds exactly like g * c and sums of squares
scale exactly.  Gradients are made in their own dtype first and then
multiplied by the current scale; with scales of 2**8 .. 2**10 and |g| < 8
fp16 stays finite.  Moments are compared as well as parameters: AdamW's
update is nearly scale-invariant and would hide a missing unscale.
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers
from tests.test_gpu_fused_steps import (_copy, _randn, _same_bits, _tuple,
                                        edge_tuples, many_tuples)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

FORMS = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}
OPTS = ["sgd", "adamw", "lamb"]
S = 2.0 ** 8


@pytest.fixture(scope="module", autouse=True)
def _device():
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    yield


# ---- the step kernels with `skip` -------------------------------------------

def sweep_tuples():
    """One tensor of 40 000 elements: SGD's and AdamW's 16 blocks of 256
    lanes take 16 384 (fp32) or 32 768 (master form) elements per sweep, so
    every form runs a second grid-stride sweep."""
    return [_tuple(40000, 77)]


LISTS = {"edge": edge_tuples, "capacity": many_tuples, "sweep": sweep_tuples}


def _low(x, lp):
    """x in the 2-byte dtype, unaligned where x is."""
    if x.data_ptr() % 16 == 0:
        return x.to(lp)
    y = torch.cat([x.new_zeros(1), x]).to(lp)[1:]
    assert y.data_ptr() % 16 != 0
    return y


def _form(tuples, lp):
    """fp32 tuples (p, g, m, v) -> rows (w, g, m, v, q): with `lp` w is the
    fp32 master, g the 2-byte gradient and q the 2-byte model parameter;
    without, q is absent."""
    if lp is None:
        return [list(t) for t in tuples]
    return [[t[0], _low(t[1], lp), t[2], t[3], _low(t[0], lp)]
            for t in tuples]


def _call(opt, rows, coef=None, skip="absent"):
    """One _core step; skip="absent" leaves the keyword out.  -> LAMB's
    trust ratios, else None."""
    from horovod_amd import _core
    col = lambda k: [r[k] for r in rows]                      # noqa: E731
    models = col(4) if len(rows[0]) == 5 else None
    kw = {} if isinstance(skip, str) else {"skip": skip}
    if opt == "sgd":
        return _core.fused_sgd_step(col(0), col(1), col(2), 0.1, 0.9, 0.01,
                                    0.0, True, coef, models, **kw)
    if opt == "adamw":
        return _core.fused_adamw_step(col(0), col(1), col(2), col(3), 1e-2,
                                      0.9, 0.95, 1e-8, 0.05, 3, coef, models,
                                      **kw)
    return _core.fused_lamb_step(col(0), col(1), col(2), col(3), 1e-2, 0.9,
                                 0.95, 1e-6, 0.05, 3, True, True, coef,
                                 models, **kw)


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _rows_equal(a, b):
    return all(torch.equal(_bits(x), _bits(y))
               for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@requires_gpu
@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("opt", OPTS)
def test_skip_flag_on_the_step_kernels(opt, form, which):
    before = _form(LISTS[which](), FORMS[form])
    coef = torch.full((1,), 0.25, device="cuda")
    # set: every row as it was, LAMB's ratios defined
    got = _copy(before)
    trust = _call(opt, got, coef, torch.ones(1, device="cuda"))
    assert _rows_equal(got, before), "a skipped step must touch nothing"
    if opt == "lamb":
        assert trust.tolist() == [1.0] * len(before)
    # clear: the call without the keyword, bit for bit
    plain, zero = _copy(before), _copy(before)
    t_plain = _call(opt, plain, coef)
    t_zero = _call(opt, zero, coef, torch.zeros(1, device="cuda"))
    assert _rows_equal(zero, plain)
    if opt == "lamb":
        assert _same_bits(t_zero, t_plain)
    assert not _rows_equal(plain, before), "the step did something"
    # a NaN flag is nonzero
    got = _copy(before)
    _call(opt, got, coef, torch.full((1,), float("nan"), device="cuda"))
    assert _rows_equal(got, before)


@requires_gpu
@pytest.mark.parametrize("opt", OPTS)
def test_skip_is_validated_before_any_launch(opt):
    rows = _form([_tuple(8, 1)], None)
    keep = _copy(rows)
    for bad in (torch.zeros(1), torch.zeros(2, device="cuda"),
                torch.zeros(1, device="cuda", dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="skip"):
            _call(opt, rows, None, bad)
    assert _rows_equal(rows, keep)


# ---- the scaled norm pass ---------------------------------------------------

def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _dev(x, dtype=torch.float32):
    return torch.tensor(x, dtype=dtype, device="cuda")


@requires_gpu
def test_scaled_norm_closed_form():
    from horovod_amd import _core
    norm = _core.multi_tensor_scaled_grad_norm
    small = [torch.full((16,), 0.25 * S, device="cuda")]   # norm exactly S
    scale = _dev(S)
    # no clip: coef is the reciprocal of the scale
    assert norm(small, None, scale).tolist() == [1.0, 1 / S, 0.0, S]
    assert norm(small, 1e4, scale).tolist() == [1.0, 1 / S, 0.0, S]
    # active clip, by clip_finalize_k's fp32 arithmetic on the unscaled norm
    clip = (_f32(1.0) / (_f32(1.0) + _f32(1e-6))) * _f32(0.5)
    assert norm(small, 0.5, scale).tolist() == \
        [1.0, (clip * _f32(1 / S)).item(), 0.0, S]
    # no scale: S = 1, and the plain entry point's {norm, coef}
    plain = _core.multi_tensor_grad_norm(small, 0.5).tolist()
    assert norm(small, 0.5).tolist() == plain + [0.0, 1.0]
    # nothing to reduce
    assert norm([], 1.0, scale).tolist() == [0.0, 1 / S, 0.0, S]
    empty = [torch.empty(0, device="cuda")]
    assert norm(empty, None).tolist() == [0.0, 1.0, 0.0, 1.0]
    # an external flag alone sets found
    assert norm(small, None, scale, _dev(1.0)).tolist() == \
        [1.0, 1 / S, 1.0, S]
    assert scale.item() == S, "no tracker: the scale is only read"
    # a finite norm above sqrt(FLT_MAX) counts as overflow
    huge = [torch.full((4,), 1e19, device="cuda")] * 4
    out = norm(huge, None, scale)
    assert out[2].item() == 1.0 and torch.isinf(out[0])


def _norm_inputs(dtype):
    """-> tensors and the (tensor, element) positions to poison: the 16-byte
    loop and the scalar tail of an aligned tensor, the last element of an
    unaligned tensor (all scalar loop), the third chunk of a 20 000-element
    tensor, tensor 60 of 100 (second batch)."""
    def mk(n, seed, offset=0):
        return _randn((n + offset,), seed).to(dtype)[offset:]
    ts = [mk(5 + (7 * i) % 36, 500 + i) for i in range(100)]
    ts[0] = mk(4097, 1)
    ts[1] = mk(1029, 2, offset=1)
    ts[2] = mk(20000, 3)
    assert ts[0].data_ptr() % 16 == 0 and ts[1].data_ptr() % 16 != 0
    return ts, [(0, 8), (0, 4096), (1, 1028), (2, 2 * 8192 + 100), (60, 3)]


@requires_gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_scaled_norm_finds_every_non_finite_element(form):
    from horovod_amd import _core
    dtype = FORMS[form] or torch.float32
    ts, positions = _norm_inputs(dtype)
    scale = _dev(S)
    clean = _core.multi_tensor_scaled_grad_norm(ts, 1.0, scale)
    assert clean[2].item() == 0.0 and clean[0].item() > 0
    # no atomics: two calls give the same bits, whatever the workspace held
    junk = torch.full((4096,), float("nan"), device="cuda")
    del junk
    again = _core.multi_tensor_scaled_grad_norm(ts, 1.0, scale)
    assert _same_bits(clean, again)
    found = []
    for t, i in positions:
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = ts[t][i].clone()
            ts[t][i] = bad
            found.append(_core.multi_tensor_scaled_grad_norm(
                ts, 1.0, scale)[2:3])
            ts[t][i] = keep
    assert torch.cat(found).tolist() == [1.0] * 15
    last = _core.multi_tensor_scaled_grad_norm(ts, 1.0, scale)
    assert _same_bits(clean, last)


@requires_gpu
def test_scale_and_tracker_follow_torch_amp_update_scale():
    """In-place update on the device against torch._amp_update_scale_ on the
    CPU, over a scripted run of flags (external, and once a real inf)."""
    from horovod_amd import _core
    flags = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    g = [_randn((100,), 9) * S]
    scale, tracker = _dev(S), _dev(0, torch.int32)
    ref_scale, ref_tracker = _f32(S), torch.tensor(0, dtype=torch.int32)
    for call, flag in enumerate(flags):
        before = scale.item()
        if call == 6:           # a real overflow instead of the external flag
            bad = [g[0].clone()]
            bad[0][50] = float("inf")
            out = _core.multi_tensor_scaled_grad_norm(
                bad, None, scale, None, tracker, 2.0, 0.5, 2)
        else:
            out = _core.multi_tensor_scaled_grad_norm(
                g, None, scale, _dev(float(flag)), tracker, 2.0, 0.5, 2)
        torch._amp_update_scale_(ref_scale, ref_tracker, _f32(float(flag)),
                                 2.0, 0.5, 2)
        # the values of this step belong to the scale before the update
        assert out[3].item() == before and out[2].item() == flag
        assert out[1].item() == 1 / before
        assert scale.item() == ref_scale.item(), call
        assert tracker.item() == ref_tracker.item(), call
    # growth that would overflow keeps the scale and restarts the count
    scale, tracker = _dev(2.0 ** 127), _dev(1, torch.int32)
    _core.multi_tensor_scaled_grad_norm([], None, scale, None, tracker, 2.0,
                                        0.5, 2)
    assert scale.item() == 2.0 ** 127 and tracker.item() == 0


@requires_gpu
def test_scaled_norm_is_validated_before_any_launch():
    from horovod_amd import _core
    norm = _core.multi_tensor_scaled_grad_norm
    g = [torch.ones(8, device="cuda")]
    scale, tracker = _dev(S), _dev(0, torch.int32)
    with pytest.raises(RuntimeError, match="scale"):
        norm(g, None, torch.tensor(S))
    with pytest.raises(RuntimeError, match="found_inf"):
        norm(g, None, scale, torch.zeros(2, device="cuda"))
    with pytest.raises(RuntimeError, match="growth_tracker"):
        norm(g, None, scale, None, _dev(0, torch.int64), 2.0, 0.5, 2)
    with pytest.raises(RuntimeError, match="needs a scale"):
        norm(g, None, None, None, tracker, 2.0, 0.5, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        norm([torch.ones(8, device="cuda"), torch.ones(8)], None, scale, None,
             tracker, 2.0, 0.5, 2)
    assert scale.item() == S and tracker.item() == 0


# ---- the optimizers ---------------------------------------------------------

SHAPES = [(33,), (128, 64), (7, 3, 3), (1029,)]
OPT_KW = {
    "sgd": dict(lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True),
    "adamw": dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05),
    "lamb": dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.05),
}
DYNAMIC = dict(loss_scale="dynamic", loss_scale_args=dict(
    init_scale=S, growth_interval=2))
MODES = {"static": dict(loss_scale=S), "dynamic": DYNAMIC}
# the scale each of six calls sees, an inf in call 3: growth after two clean
# steps, backoff after the overflow
SCALES = {"static": [S] * 6,
          "dynamic": [S, S, 2 * S, S, S, 2 * S]}
STATE_KEYS = ("master_param", "exp_avg", "exp_avg_sq", "momentum_buffer")


def _make(opt, params, **extra):
    from horovod_amd.ops import FusedAdamW, FusedLAMB, FusedSGD
    cls = {"sgd": FusedSGD, "adamw": FusedAdamW, "lamb": FusedLAMB}[opt]
    return cls(params, **dict(OPT_KW[opt], **extra))


def _params(dtype, seed=5, shapes=SHAPES):
    return [_randn(s, seed + i).to(dtype).requires_grad_(True)
            for i, s in enumerate(shapes)]


def _grads(call, dtype, shapes=SHAPES):
    return [_randn(s, 1000 + 10 * call + i).to(dtype)
            for i, s in enumerate(shapes)]


def _same_state(a, ps, b, qs):
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), i
        sa, sb = a.state[p], b.state[q]
        assert set(sa) == set(sb)
        for key in sa:
            if torch.is_tensor(sa[key]) and sa[key].dim() > 0:
                assert torch.equal(_bits(sa[key]), _bits(sb[key])), (i, key)
            else:
                assert int(sa[key]) == int(sb[key]), (i, key)
        if "master_param" in sa:
            assert torch.equal(p.detach(), sa["master_param"].to(p.dtype))


def _scaled_run(opt, dtype, mode, extra, ps, qs, calls=6, bad_call=2,
                bad_param=0):
    """Six calls of the scaled optimizer on ps, an inf in call 3; the plain
    one on qs gets the other five gradient sets.  -> the two optimizers."""
    scaled = _make(opt, ps, **dict(MODES[mode], **extra))
    plain = _make(opt, qs, **extra)
    for call in range(calls):
        scale = scaled.get_loss_scale()
        assert scale == SCALES[mode][call], (call, scale)
        assert scaled.loss_scale_tensor.item() == scale
        grads = _grads(call, dtype)
        for p, g in zip(ps, grads):
            p.grad = g * scale
            assert p.grad.dtype == dtype and torch.isfinite(p.grad).all()
        if call == bad_call:
            ps[bad_param].grad.view(-1)[3] = float("inf")
        fed = [p.grad.clone() for p in ps]
        before = [p.detach().clone() for p in ps]
        scaled.step()
        for p, g in zip(ps, fed):
            assert torch.equal(_bits(p.grad), _bits(g)), \
                "step() must not write p.grad"
        assert scaled.last_found_inf.item() == (call == bad_call)
        if call == bad_call:
            for p, b in zip(ps, before):
                assert torch.equal(_bits(p.detach()), _bits(b))
            continue
        for q, g in zip(qs, grads):
            q.grad = g
        plain.step()
        if extra.get("max_grad_norm") is not None:
            assert _same_bits(scaled.last_grad_norm.reshape(1),
                              plain.last_grad_norm.reshape(1)), call
        assert not torch.equal(ps[0].detach(), before[0])
    return scaled, plain


@requires_gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clip", [None, 1.0, 1e4], ids=["noclip", "clip",
                                                         "inactive"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("opt", OPTS)
def test_scaled_optimizer_equals_plain_bitwise(opt, form, clip, mode):
    dtype = FORMS[form] or torch.float32
    extra = dict(max_grad_norm=clip, master_weights=form != "fp32")
    ps, qs = _params(dtype), _params(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no eager fallback here
        scaled, plain = _scaled_run(opt, dtype, mode, extra, ps, qs)
        sd = scaled.state_dict()                # settles the last step
    _same_state(scaled, ps, plain, qs)
    assert scaled.skipped_steps == 1
    if opt != "sgd":
        assert all(int(scaled.state[p]["step"]) == 5 for p in ps)
    assert sd["loss_scaler"] == {
        "scale": SCALES[mode][-1],
        "growth_tracker": 1 if mode == "dynamic" else 0}
    assert "loss_scaler" not in plain.state_dict()


@requires_gpu
@pytest.mark.parametrize("bad_param", [0, 2], ids=["inf_in_fused",
                                                   "inf_in_eager"])
@pytest.mark.parametrize("opt", OPTS)
def test_mixed_group_skips_as_a_whole(opt, bad_param):
    """A bf16 parameter without master weights takes the eager update, the
    fp32 ones the kernels; an overflow in either skips both."""
    def params():
        ps = _params(torch.float32)
        ps[2] = ps[2].detach().bfloat16().requires_grad_(True)
        return ps

    ps, qs = params(), params()
    scaled = _make(opt, ps, **DYNAMIC)
    plain = _make(opt, qs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call in range(4):
            scale = scaled.get_loss_scale()
            grads = [g.to(p.dtype) for g, p in
                     zip(_grads(call, torch.float32), ps)]
            for p, g in zip(ps, grads):
                p.grad = g * scale
            before = [p.detach().clone() for p in ps]
            if call == 2:
                ps[bad_param].grad.view(-1)[0] = float("nan")
                scaled.step()
                for p, b in zip(ps, before):
                    assert torch.equal(_bits(p.detach()), _bits(b))
                continue
            scaled.step()
            for q, g in zip(qs, grads):
                q.grad = g
            plain.step()
    assert scaled.get_loss_scale() == S       # grown, then halved
    assert scaled.skipped_steps == 1
    _same_state(scaled, ps, plain, qs)


@requires_gpu
@pytest.mark.parametrize("opt", OPTS)
def test_state_dict_round_trip_continues_bitwise(opt):
    ps, qs = _params(torch.float16), _params(torch.float16)
    extra = dict(master_weights=True, max_grad_norm=1.0)
    scaled, _ = _scaled_run(opt, torch.float16, "dynamic", extra, ps, qs,
                            calls=4)
    sd = scaled.state_dict()
    assert sd["loss_scaler"] == {"scale": S, "growth_tracker": 1}
    rs = [p.detach().clone().requires_grad_(True) for p in ps]
    loaded = _make(opt, rs, **dict(DYNAMIC, **extra))
    loaded.load_state_dict(sd)
    assert loaded.get_loss_scale() == S
    # a dict without the entry keeps what is there
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


@requires_gpu
def test_scale_loss_and_option_errors():
    p = _params(torch.float32)[:1]
    opt = _make("adamw", p, **DYNAMIC)
    loss = torch.full((), 3.0, device="cuda")
    assert opt.scale_loss(loss).item() == 3.0 * S
    assert opt.loss_scale_tensor.dim() == 0
    assert opt.loss_scale_tensor.device == p[0].device
    with pytest.raises(RuntimeError, match="loss_scale"):
        _make("adamw", p).scale_loss(loss)


# ---- torch.amp.GradScaler ---------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
def test_grad_scaler_steps_fp16_master_parameters(clip):
    """GradScaler.step() refuses fp16 gradients of an optimizer that does
    not do the unscaling itself.  Here it hands scale and flag to step():
    fp16 master-weight parameters step, an overflow skips, and the fp32
    trajectory is torch.optim.AdamW's under the same scaler settings."""
    from horovod_amd.ops import FusedAdamW
    kw = OPT_KW["adamw"]

    def scaler():
        return torch.amp.GradScaler("cuda", init_scale=S, growth_interval=2)

    # fp16 + master against the plain optimizer on unscaled gradients
    ps, qs = _params(torch.float16), _params(torch.float16)
    opt = FusedAdamW(ps, master_weights=True, max_grad_norm=clip, **kw)
    plain = FusedAdamW(qs, master_weights=True, max_grad_norm=clip, **kw)
    sc = scaler()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for call in range(5):
            scale = sc.scale(torch.ones((), device="cuda")).item()
            assert scale == [S, S, 2 * S, S, S][call]
            grads = _grads(call, torch.float16)
            for p, g in zip(ps, grads):
                p.grad = g * scale
            if call == 2:
                ps[1].grad[0, 0] = float("inf")
            sc.step(opt)
            sc.update()
            if call != 2:
                for q, g in zip(qs, grads):
                    q.grad = g
                plain.step()
    opt.state_dict()
    assert opt.skipped_steps == 1
    assert all(opt.state[p]["step"] == 4 for p in ps)
    _same_state(opt, ps, plain, qs)

    # fp32 against torch.optim.AdamW + GradScaler
    ps, qs = _params(torch.float32), _params(torch.float32)
    opt = FusedAdamW(ps, max_grad_norm=clip, **kw)
    ref = torch.optim.AdamW(qs, **kw)
    sc, sc_ref = scaler(), scaler()
    for call in range(5):
        scale = sc.scale(torch.ones((), device="cuda")).item()
        assert sc_ref.scale(torch.ones((), device="cuda")).item() == scale
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
    assert not torch.equal(ps[0].detach(), _params(torch.float32)[0])


@requires_gpu
def test_grad_scaler_and_loss_scale_option_exclude_each_other():
    ps = _params(torch.float32)[:1]
    opt = _make("adamw", ps, **DYNAMIC)
    sc = torch.amp.GradScaler("cuda", init_scale=S)
    sc.scale(torch.ones((), device="cuda"))
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(RuntimeError, match="GradScaler"):
        sc.step(opt)


# ---- asynchrony -------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("opt", OPTS)
def test_first_scaled_step_does_not_synchronise(opt):
    ps = _params(torch.float16)
    grads = [g * S for g in _grads(0, torch.float16)]
    optimizer = _make(opt, ps, master_weights=True, max_grad_norm=1.0,
                      **DYNAMIC)
    probe = torch.ones((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            guarded = False
        except RuntimeError:
            guarded = True
        if guarded:
            loss = optimizer.scale_loss(probe)
            for p, g in zip(ps, grads):
                p.grad = g
            optimizer.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not guarded:
        pytest.skip(".item() does not raise under set_sync_debug_mode('error')"
                    " on this build")
    assert loss.item() == S
    assert optimizer.get_loss_scale() == S and optimizer.skipped_steps == 0
    assert all(int(optimizer.state[p]["step"]) == 1 for p in ps
               if "step" in optimizer.state[p])


# ---- two ranks --------------------------------------------------------------

TWO_RANK_BODY = """
        from horovod_amd.ops import FusedAdamW
        dev = torch.device("cuda",
                           hvd.local_rank() % torch.cuda.device_count())
        torch.cuda.set_device(dev)
        shapes = [(33,), (128, 64), (7, 3, 3), (1029,)]
        S = 2.0 ** 8

        def randn(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).to(dev) for s in shapes]

        def same_on_all_ranks(ts, name):
            # both ranks share one GPU, so the bits travel as host tensors
            mine = torch.cat([t.detach().reshape(-1) for t in ts]).cpu()
            both = hvd.allgather(mine.view(torch.int32).reshape(1, -1),
                                 name=name)
            assert both.shape[0] == size and bool((both == both[0]).all())

        ps = [p.requires_grad_(True) for p in randn(1)]   # same on all ranks
        start = [p.detach().clone() for p in ps]
        opt = hvd.DistributedOptimizer(
            FusedAdamW(ps, lr=1e-2, max_grad_norm=1.0, loss_scale="dynamic",
                       loss_scale_args=dict(init_scale=S, growth_interval=2)),
            named_parameters=[(f"p{i}", p) for i, p in enumerate(ps)])
        assert all(g["loss_scale"] == "dynamic" for g in opt.param_groups)
        # only rank 1 overflows; the flag comes from the reduced gradients
        for p, g in zip(ps, randn(50 + rank)):
            p.grad = g * opt.get_loss_scale()
        if rank == 1:
            ps[1].grad[3, 3] = float("inf")
        opt.step()
        assert opt.last_found_inf.item() == 1.0
        assert opt.get_loss_scale() == S / 2 and opt.skipped_steps == 1
        for p, p0 in zip(ps, start):
            assert torch.equal(p.detach(), p0)
            assert "step" not in opt.state[p] or opt.state[p]["step"] == 0
        # and a clean step on the halved scale
        for p, g in zip(ps, randn(60 + rank)):
            p.grad = g * opt.get_loss_scale()
        opt.step()
        assert opt.get_loss_scale() == S / 2 and opt.skipped_steps == 1
        assert all(opt.state[p]["step"] == 1 for p in ps)
        assert not torch.equal(ps[0].detach(), start[0])
        same_on_all_ranks(ps, "ls.params")
        same_on_all_ranks([opt.last_grad_norm.reshape(1)], "ls.norm")
"""


@requires_gpu
def test_two_ranks_one_overflows_both_skip():
    """Through hvd.DistributedOptimizer with no manual synchronize: the norm
    pass runs on the reduced gradients, so one rank's inf skips the step and
    halves the scale on both."""
    run_workers(2, TWO_RANK_BODY,
                extra_env={"HOROVOD_ONESHOT_ALLREDUCE": "1"}, timeout=300)
