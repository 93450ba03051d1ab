"""GPU tests (MI355X) for FusedLARS and the three LARS kernels
(csrc/lars_kernels.hip): norms, trust ratios, update.

The reference is the fp64 evaluation of the definition from
tests/test_lars_build.py (RefLars), independent of fused_lars.py; inputs and
tolerances are the ones documented there.  The direct kernel calls use the
edge list and the 100-tensor list of test_gpu_lamb.py as (p, g, m) triples.

Master weights and loss scaling are held to the plain fp32 path bit for bit:
the norm pass sums in one order whatever the gradient's dtype and alignment,
widening a 2-byte gradient is exact, and for a power-of-two scale S
(S * g) * (c / S) rounds exactly like g * c.
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers
from tests.test_lars_build import (ATOL, CASES, KW, RTOL, STEPS, RefLars,
                                   check_spread)
from tests.test_lars_build import _grads as _cpu_grads
from tests.test_lars_build import _params as _cpu_params

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

LOW = {"fp16": torch.float16, "bf16": torch.bfloat16}
FORMS = {"fp32": None, **LOW}


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


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _rows_equal(a, b):
    return all(_same_bits(x, y) for ra, rb in zip(a, b)
               for x, y in zip(ra, rb))


def _copy(tuples):
    return [[x.clone() for x in t] for t in tuples]


def _close(p, q, where):
    p = p.detach().double()
    assert torch.allclose(p, q, rtol=RTOL, atol=ATOL, equal_nan=True), \
        (where, (p - q).abs().max().item())


def _follow(opt, ps, ref, steps=STEPS, grads_of=_grads):
    for step in range(steps):
        grads = grads_of(step)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref.step(grads)
        for p, g in zip(ps, grads):
            # bitwise, so that a NaN put there on purpose compares equal
            assert _same_bits(p.grad, g), "step() must not scale p.grad"
        for i, (p, q) in enumerate(zip(ps, ref.p)):
            _close(p, q, (step, i))


# ---- optimizer trajectories -----------------------------------------------

@requires_gpu
def test_fused_lars_matches_fp64():
    from horovod_amd.ops import FusedLARS
    ps = _params()
    ref = RefLars(ps, **KW)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # no eager fallback here
        opt = FusedLARS(ps, **KW)
        _follow(opt, ps, ref)
    # a trust ratio of 1 everywhere would be far outside the tolerance
    check_spread("plain", ref.trust)
    for p, m in zip(ps, ref.m):
        assert opt.state[p]["momentum_buffer"].dtype == torch.float32
        _close(opt.state[p]["momentum_buffer"], m, "m")
    assert all(not torch.equal(p.detach().cpu(), p0.detach())
               for p, p0 in zip(ps, _cpu_params()))


@requires_gpu
@pytest.mark.parametrize("case", [c for c in CASES if c != "plain"])
def test_options_follow_definition(case):
    from horovod_amd.ops import FusedLARS
    kw = dict(KW, **CASES[case])
    ps = _params()
    ref = RefLars(ps, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt = FusedLARS(ps, **kw)
        _follow(opt, ps, ref, steps=3)
    check_spread(case, ref.trust)
    for p, m in zip(ps, ref.m):
        _close(opt.state[p]["momentum_buffer"], m, (case, "m"))
    if case == "clip":
        assert ref.norm > 90, "clip must be active"
        assert abs(opt.last_grad_norm.item() - ref.norm) <= 1e-5 * ref.norm


@requires_gpu
def test_no_decay_group_is_fused_sgd_bitwise():
    """weight_decay=0 without always_adapt: trust is exactly 1 and the
    per-element arithmetic is sgd_element's, so FusedSGD is the oracle."""
    from horovod_amd.ops import FusedLARS, FusedSGD
    ps, qs = _params(), _params()
    lars = FusedLARS(ps, lr=0.1, momentum=0.9)
    sgd = FusedSGD(qs, lr=0.1, momentum=0.9)
    for step in range(3):
        for p, q, g in zip(ps, qs, _grads(step)):
            p.grad = g.clone()
            q.grad = g.clone()
        lars.step()
        sgd.step()
    for p, q in zip(ps, qs):
        assert _same_bits(p.detach(), q.detach())
        assert _same_bits(lars.state[p]["momentum_buffer"],
                          sgd.state[q]["momentum_buffer"])


# ---- direct kernel calls --------------------------------------------------

HYPER = dict(lr=0.5, momentum=0.9, trust_coefficient=0.02, eps=1e-8,
             nesterov=False, trust_clip=False, adapt=True)


def _triple(n, seed, scale=1.0, offset=0):
    """(p, g, m) of n elements; offset=1 makes views that are not 16-byte
    aligned."""
    def mk(s, sc):
        return _randn((n + offset,), s, sc)[offset:]
    return [mk(seed, scale), mk(seed + 1, 1.0), mk(seed + 2, 0.1)]


def _edge_triples():
    # parameter scales spread the ratios so a mixed-up index shows
    ts = [_triple(n, 10 * n, sc) for n, sc in
          [(0, 1.0), (1, 20.0), (3, 0.05), (33, 1.0), (4097, 20.0)]]
    ts.append(_triple(1029, 7, 0.05, offset=1))
    assert all(t.data_ptr() % 16 != 0 for t in ts[-1])
    ts.append(_triple(20000, 8))         # three chunks, ragged last one
    zero_p = _triple(100, 9)
    zero_p[0].zero_()                    # |p| = 0: trust 1
    ts.append(zero_p)
    zero_g = _triple(100, 11)
    zero_g[1].zero_()                    # g = 0: trust 1
    ts.append(zero_g)
    return ts


def _many_triples():
    """100 tensors of 5..40 elements: crosses the 48-descriptor capacity
    twice; the scales spread the ratios so a wrong index shows."""
    return [_triple(5 + (7 * i) % 36, 200 + 4 * i, (0.05, 1.0, 20.0)[i % 3])
            for i in range(100)]


LISTS = {"edge": _edge_triples, "100_tensors": _many_triples}


def _ref_direct(triples, weight_decay, hyper=HYPER):
    ref = RefLars([t[0] for t in triples], hyper["lr"], hyper["momentum"],
                  weight_decay, hyper["trust_coefficient"], hyper["eps"],
                  hyper["nesterov"], hyper["trust_clip"])
    ref.adapt = hyper["adapt"]
    ref.m = [t[2].double() for t in triples]
    ref.step([t[1] for t in triples])
    return ref


def _torch_trust(t, weight_decay, hyper=HYPER):
    """The ratio formed with fp32 torch ops and vector_norm."""
    wn = torch.linalg.vector_norm(t[0])
    gn = torch.linalg.vector_norm(t[1])
    r = hyper["trust_coefficient"] * wn / (gn + weight_decay * wn +
                                           hyper["eps"])
    if hyper["trust_clip"]:
        r = torch.clamp(r / hyper["lr"], max=1.0)
    return r.item()


def _call(rows, weight_decay, hyper=HYPER, grad_coef=None, skip="absent"):
    """rows: (p, g, m) or, master weights, (p, g, m, model)."""
    from horovod_amd import _core
    col = lambda k: [r[k] for r in rows]                      # noqa: E731
    kw = {} if isinstance(skip, str) else {"skip": skip}
    models = col(3) if rows and len(rows[0]) == 4 else None
    return _core.fused_lars_step(col(0), col(1), col(2),
                                 weight_decay=weight_decay,
                                 grad_coef=grad_coef, model_params=models,
                                 **hyper, **kw)


def _check_direct(triples, weight_decay, label, hyper=HYPER):
    before = _copy(triples)
    ref = _ref_direct(before, weight_decay, hyper)
    trust = _call(triples, weight_decay, hyper)
    assert trust.dtype == torch.float32 and trust.shape == (len(triples),)
    assert trust.is_cuda
    trust = trust.tolist()
    worst = (0.0, 0.0)
    for i, (t, b) in enumerate(zip(triples, before)):
        assert _same_bits(t[1], b[1]), "gradients are only read"
        _close(t[0], ref.p[i], (label, i, "p"))
        _close(t[2], ref.m[i], (label, i, "m"))
        want = ref.trust[i]
        if want == 1.0:                  # the rule's 'otherwise' branch
            assert trust[i] == 1.0, (label, i, trust[i])
            continue
        err = abs(trust[i] - want) / want
        torch_err = abs(_torch_trust(b, weight_decay, hyper) - want) / want
        bound = max(4 * torch_err, 8 * 2.0 ** -23)
        worst = max(worst, (err, torch_err))
        assert err <= bound, (label, i, err, bound)
    print(f"trust[{label}, wd={weight_decay}]: worst native rel err "
          f"{worst[0]:.3e} (torch ops on that tensor {worst[1]:.3e})")
    return ref, trust


@requires_gpu
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_kernel_edge_list_vs_fp64(weight_decay):
    triples = _edge_triples()
    ref, trust = _check_direct(triples, weight_decay, "edge")
    assert trust[0] == 1.0                       # empty tensor
    assert trust[-2] == 1.0                      # |p| = 0
    assert trust[-1] == 1.0                      # g = 0
    assert not any(torch.isnan(x).any() for t in triples for x in t)
    assert min(ref.trust) < 2e-3 and max(ref.trust) > 0.1, ref.trust


@requires_gpu
def test_kernel_100_tensors_vs_fp64():
    ref, trust = _check_direct(_many_triples(), 0.01, "100_tensors")
    assert min(ref.trust) < 2e-3 and max(ref.trust) > 0.1, ref.trust


@requires_gpu
def test_kernel_variants_vs_fp64():
    """nesterov, trust_clip (two of three tensors clip to 1) and momentum 0
    through the direct call."""
    for extra in (dict(nesterov=True), dict(trust_clip=True, lr=0.01),
                  dict(momentum=0.0)):
        hyper = dict(HYPER, **extra)
        triples = [_triple(33, 40, 0.05), _triple(4097, 50, 20.0),
                   _triple(20000, 60, 3.0)]
        ref, trust = _check_direct(triples, 0.01, str(extra), hyper)
        if "trust_clip" in extra:
            assert trust[1:] == [1.0, 1.0] and 0.05 < trust[0] < 0.5, trust


@requires_gpu
def test_kernel_without_adapt_and_with_coef():
    """adapt=False gives trust 1 whatever the norms; a grad_coef of 0.25
    equals a gradient scaled by 0.25 beforehand."""
    hyper = dict(HYPER, adapt=False)
    before = [_triple(n, 30 + n) for n in (33, 4097)]
    triples = _copy(before)
    ref = _ref_direct(before, 0.01, hyper)
    trust = _call(triples, 0.01, hyper)
    assert trust.tolist() == [1.0, 1.0] and ref.trust == [1.0, 1.0]
    for i, t in enumerate(triples):
        _close(t[0], ref.p[i], (i, "p"))

    before = _edge_triples() + _many_triples()
    coef = torch.full((1,), 0.25, device="cuda")
    a, b = _copy(before), _copy(before)
    for t in b:
        t[1] = t[1] * 0.25
    ta, tb = _call(a, 0.01, grad_coef=coef), _call(b, 0.01)
    assert _same_bits(ta, tb)
    for x, y, orig in zip(a, b, before):
        assert _same_bits(x[1], orig[1]), "gradients are only read"
        for k in (0, 2):
            assert _same_bits(x[k], y[k])
    assert not _rows_equal(a, before)


@requires_gpu
def test_kernel_rejects_bad_inputs():
    from horovod_amd import _core
    ok = _triple(8, 1)

    def call(p, g, m):
        _core.fused_lars_step([p], [g], [m], weight_decay=0.01, **HYPER)

    keep = ok[0].clone()
    with pytest.raises(RuntimeError, match="fp32"):
        call(ok[0], ok[1].half(), ok[2])       # fp16 without model_params
    with pytest.raises(RuntimeError, match="GPU"):
        call(ok[0], ok[1].cpu(), ok[2])
    with pytest.raises(RuntimeError, match="size"):
        call(ok[0], ok[1][:7], ok[2])
    with pytest.raises(RuntimeError, match="dense"):
        call(ok[0], _randn((16,), 2)[::2], ok[2])
    with pytest.raises(RuntimeError, match="as many"):
        _core.fused_lars_step([ok[0]], [], [ok[2]], weight_decay=0.01,
                              **HYPER)
    with pytest.raises(RuntimeError, match="as many"):
        _core.fused_lars_step([ok[0]], [ok[1]], [], weight_decay=0.01,
                              **HYPER)
    assert torch.equal(ok[0], keep), "a rejected call must not launch"
    out = _core.fused_lars_step([], [], [], weight_decay=0.01, **HYPER)
    assert out.shape == (0,) and out.dtype == torch.float32


@requires_gpu
def test_kernel_deterministic():
    """No atomics: the same inputs give bitwise the same trust ratios and
    tensors, whatever the workspace held before."""
    base = _edge_triples() + _many_triples()
    runs = []
    for k in range(3):
        triples = _copy(base)
        runs.append((_call(triples, 0.01), triples))
        # the next call's workspace comes back from the caching allocator
        # with this call's partials, or with garbage, in it
        junk = torch.full((4096,), float("nan"), device="cuda")
        del junk
    for trust, triples in runs[1:]:
        assert _same_bits(trust, runs[0][0])
        assert _rows_equal(triples, runs[0][1])
    assert not _rows_equal(runs[0][1], base)


# ---- master weights -------------------------------------------------------

def _low(x, lp, offset=None):
    """x in the 2-byte dtype, `offset` elements into its storage (default:
    one element, i.e. unaligned, where x is unaligned)."""
    if offset is None:
        offset = 0 if x.data_ptr() % 16 == 0 else 1
    y = torch.cat([x.new_zeros(offset), x]).to(lp)[offset:]
    assert y.data_ptr() % 16 == (2 * offset) % 16
    return y


def _master_rows(triples, dtypes, lp_offsets=None):
    """-> fp32 rows (p, widened g, m) and master rows (p, g_lp, m, model)
    over the same values; model starts as junk the kernel must overwrite."""
    lp_offsets = lp_offsets or {}
    fp32, master = [], []
    for i, (t, dt) in enumerate(zip(triples, dtypes)):
        g_lp = _low(t[1], dt, lp_offsets.get(i))
        g32 = g_lp.float()
        if t[1].data_ptr() % 16 != 0:           # keep the fp32 row unaligned
            g32 = torch.cat([g32.new_zeros(1), g32])[1:]
        fp32.append([t[0].clone(), g32, t[2].clone()])
        master.append([t[0].clone(), g_lp, t[2].clone(),
                       _low(torch.full_like(t[0], 7.0), dt,
                            lp_offsets.get(i))])
    return fp32, master


@requires_gpu
@pytest.mark.parametrize("which,low", [("edge", "fp16"), ("edge", "bf16"),
                                       ("100_tensors", "fp16"),
                                       ("100_tensors", "bf16"),
                                       ("100_tensors", "mixed")])
def test_master_kernel_bitwise_fp32_kernel(which, low):
    triples = LISTS[which]()
    offsets = {}
    if which == "edge":
        # fp32 rows 16-byte aligned, 2-byte rows 8 bytes off: the norm pass
        # still loads quads, the update runs element by element
        triples.append(_triple(1029, 3))
        offsets[len(triples) - 1] = 4
    dts = [(torch.float16, torch.bfloat16)[i % 2] if low == "mixed"
           else LOW[low] for i in range(len(triples))]
    for coef in (None, torch.full((1,), 0.25, device="cuda")):
        fp32, master = _master_rows(triples, dts, offsets)
        lp_before = [t[1].clone() for t in master]
        t32 = _call(fp32, 0.01, grad_coef=coef)
        tm = _call(master, 0.01, grad_coef=coef)
        assert _same_bits(t32, tm), (t32 - tm).abs().max().item()
        for i, (a, b, g) in enumerate(zip(fp32, master, lp_before)):
            assert _same_bits(b[1], g), (i, "gradients are only read")
            assert _same_bits(a[0], b[0]), (i, "master")
            assert _same_bits(a[2], b[2]), (i, "momentum")
            assert _same_bits(b[3], b[0].to(b[3].dtype)), (i, "model")
        assert not torch.equal(master[-1][0], triples[-1][0])
        if coef is None:    # a quarter of the gradient: four times the ratio
            assert min(t32.tolist()) < 2e-3 and max(t32.tolist()) > 0.1


@requires_gpu
def test_mixed_group_takes_both_kernels_without_warning():
    """fp32 and bf16 parameters in one master_weights group: none takes the
    eager update, only the bf16 ones get a master, and each stays the rounded
    master."""
    from horovod_amd.ops import FusedLARS
    shapes = [(33,), (128, 24), (7, 3, 3), (1029,)]
    dts = [torch.float32, torch.bfloat16, torch.bfloat16, torch.float32]
    ps = [_randn(s, 80 + i).to(dt).requires_grad_(True)
          for i, (s, dt) in enumerate(zip(shapes, dts))]
    start = [p.detach().clone() for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt = FusedLARS(ps, master_weights=True, **KW)
        for step in range(2):
            for i, p in enumerate(ps):
                p.grad = _randn(p.shape, 90 + 10 * step + i).to(p.dtype)
            opt.step()
    for p, s in zip(ps, start):
        st = opt.state[p]
        assert not torch.equal(p.detach(), s)
        assert st["momentum_buffer"].dtype == torch.float32
        if p.dtype == torch.float32:
            assert "master_param" not in st
        else:
            assert st["master_param"].dtype == torch.float32
            assert _same_bits(p.detach(), st["master_param"].to(p.dtype))


# ---- skip flag ------------------------------------------------------------

def _form(triples, lp):
    if lp is None:
        return _copy(triples)
    return _master_rows(triples, [lp] * len(triples))[1]


@requires_gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_skip_flag(form):
    before = _form(_edge_triples() + _many_triples(), FORMS[form])
    coef = torch.full((1,), 0.25, device="cuda")
    # set: every row as it was, the ratios defined
    for flag in (1.0, float("nan")):            # a NaN flag is nonzero
        got = _copy(before)
        trust = _call(got, 0.01, grad_coef=coef,
                      skip=torch.full((1,), flag, device="cuda"))
        assert _rows_equal(got, before), "a skipped step must touch nothing"
        assert trust.tolist() == [1.0] * len(before)
    # clear: the call without the keyword, bit for bit
    plain, zero = _copy(before), _copy(before)
    t_plain = _call(plain, 0.01, grad_coef=coef)
    t_zero = _call(zero, 0.01, grad_coef=coef,
                   skip=torch.zeros(1, device="cuda"))
    assert _rows_equal(zero, plain) and _same_bits(t_zero, t_plain)
    assert not _rows_equal(plain, before), "the step did something"
    for bad in (torch.zeros(1), torch.zeros(2, device="cuda")):
        with pytest.raises(RuntimeError, match="skip"):
            _call(plain, 0.01, skip=bad)


# ---- optimizer behaviour --------------------------------------------------

@requires_gpu
def test_nan_gradient_stays_in_its_tensor():
    """No clipping, so nothing global: a NaN in one gradient reaches only
    that tensor.  Its gn is NaN, the rule's compares are false, trust is 1,
    and the NaN lands on the element it came from; every other tensor
    follows the reference."""
    from horovod_amd.ops import FusedLARS
    ps = _params()
    ref = RefLars(ps, **KW)
    opt = FusedLARS(ps, **KW)

    def grads_of(step):
        grads = _grads(step)
        if step == 1:
            grads[1][5, 7] = float("nan")
        return grads

    for step in range(3):
        _follow(opt, ps, ref, steps=1, grads_of=lambda _: grads_of(step))
        if step == 1:
            assert ref.trust[1] == 1.0
    assert torch.isnan(ps[1][5, 7]) and torch.isnan(ref.p[1][5, 7])
    assert torch.isnan(ps[1]).sum().item() == 1
    for i in (0, 2, 3, 4):
        assert not torch.isnan(ps[i]).any(), i


@requires_gpu
def test_inactive_clip_is_bitwise_noop():
    from horovod_amd.ops import FusedLARS
    ps_c, ps_n = _params(), _params()
    oc = FusedLARS(ps_c, max_grad_norm=1e4, **KW)
    on = FusedLARS(ps_n, **KW)
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


# ---- loss scaling ---------------------------------------------------------

S = 2.0 ** 8
SCALED_SHAPES = [(33,), (128, 64), (7, 3, 3), (1029,), (20000,)]
SCALED_KW = dict(KW, lr=0.1, nesterov=True)
MODES = {
    "static": (dict(loss_scale=S), [S] * 6),
    # growth after every two clean steps
    "dynamic": (dict(loss_scale="dynamic", loss_scale_args=dict(
        init_scale=S, growth_interval=2)), [S, S, 2 * S, 2 * S, 4 * S, 4 * S]),
}


def _scaled_params(dtype, seed=5):
    return [_randn(s, seed + i).to(dtype).requires_grad_(True)
            for i, s in enumerate(SCALED_SHAPES)]


def _scaled_grads(call, dtype):
    return [_randn(s, 1000 + 10 * call + i).to(dtype)
            for i, s in enumerate(SCALED_SHAPES)]


def _same_state(a, ps, b, qs):
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert _same_bits(p.detach(), q.detach()), i
        sa, sb = a.state[p], b.state[q]
        assert set(sa) == set(sb)
        for key in sa:
            assert _same_bits(sa[key], sb[key]), (i, key)
        if "master_param" in sa:
            assert torch.equal(p.detach(), sa["master_param"].to(p.dtype))


@requires_gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("form", list(FORMS))
def test_scaled_optimizer_equals_plain_bitwise(form, clip, mode):
    from horovod_amd.ops import FusedLARS
    dtype = FORMS[form] or torch.float32
    extra = dict(SCALED_KW, max_grad_norm=clip,
                 master_weights=form != "fp32")
    option, scales = MODES[mode]
    ps, qs = _scaled_params(dtype), _scaled_params(dtype)
    start = [p.detach().clone() for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no eager fallback here
        scaled = FusedLARS(ps, **dict(extra, **option))
        plain = FusedLARS(qs, **extra)
        for call in range(6):
            scale = scaled.get_loss_scale()
            assert scale == scales[call], (call, scale)
            grads = _scaled_grads(call, dtype)
            for p, q, g in zip(ps, qs, grads):
                p.grad = g * scale
                q.grad = g
                assert p.grad.dtype == dtype and torch.isfinite(p.grad).all()
            fed = [p.grad.clone() for p in ps]
            scaled.step()
            plain.step()
            for p, g in zip(ps, fed):
                assert _same_bits(p.grad, g), "step() must not write p.grad"
            assert scaled.last_found_inf.item() == 0
            if clip is not None:
                assert _same_bits(scaled.last_grad_norm.reshape(1),
                                  plain.last_grad_norm.reshape(1)), call
        scaled.state_dict()                     # settles the last step
    _same_state(scaled, ps, plain, qs)
    assert scaled.skipped_steps == 0
    assert all(not torch.equal(p.detach(), s) for p, s in zip(ps, start))


@requires_gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_overflow_skips_the_whole_step(form):
    from horovod_amd.ops import FusedLARS
    dtype = FORMS[form] or torch.float32
    option, _ = MODES["dynamic"]
    ps = _scaled_params(dtype)
    opt = FusedLARS(ps, master_weights=form != "fp32",
                    **dict(SCALED_KW, **option))

    def feed(call):
        for p, g in zip(ps, _scaled_grads(call, dtype)):
            p.grad = g * opt.get_loss_scale()

    feed(0)
    opt.step()
    before = [[p.detach().clone()] +
              [v.clone() for _, v in sorted(opt.state[p].items())]
              for p in ps]
    feed(1)
    ps[2].grad.view(-1)[3] = float("inf")
    opt.step()
    assert opt.last_found_inf.item() == 1
    after = [[p.detach()] + [v for _, v in sorted(opt.state[p].items())]
             for p in ps]
    assert _rows_equal(after, before), "a skipped step must touch nothing"
    assert opt.get_loss_scale() == S / 2
    feed(2)
    opt.step()
    assert opt.skipped_steps == 1
    assert opt.last_found_inf.item() == 0
    assert opt.get_loss_scale() == S / 2
    assert all(not _same_bits(p.detach(), b[0]) for p, b in zip(ps, before))


# ---- two ranks ------------------------------------------------------------

TWO_RANK_BODY = """
        from horovod_amd import _core
        from horovod_amd.ops import FusedLARS
        torch.cuda.set_device(hvd.local_rank() % torch.cuda.device_count())
        dev = torch.device("cuda",
                           hvd.local_rank() % torch.cuda.device_count())
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,), (20000,)]
        scales = [0.02, 0.3, 3.0, 10.0, 1.0]
        lr, mu, wd, tc, eps = 1.0, 0.9, 0.01, 0.02, 1e-8

        def randn(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).to(dev) for s in shapes]

        ps = [(p * s).requires_grad_(True)            # same on all ranks
              for p, s in zip(randn(1), scales)]
        p0 = [p.detach().double().clone() for p in ps]
        per_rank = [randn(50 + r) for r in range(size)]
        opt = hvd.DistributedOptimizer(
            FusedLARS(ps, lr=lr, momentum=mu, weight_decay=wd,
                      trust_coefficient=tc, eps=eps, max_grad_norm=1.0),
            named_parameters=[(f"p{i}", p) for i, p in enumerate(ps)])
        assert all(g["max_grad_norm"] == 1.0 and
                   g["trust_coefficient"] == tc for g in opt.param_groups)
        for p, g in zip(ps, per_rank[rank]):
            p.grad = g.clone()
        opt.step()
        torch.cuda.synchronize()
        assert not _core.rccl_used(), "small gradients must stay one-shot"

        # the definition in fp64 on the mean gradient, first step (m = d)
        mean = [(sum(gs) / size).double() for gs in zip(*per_rank)]
        norm = torch.sqrt(sum((g * g).sum() for g in mean)).item()
        assert norm > 10, "clip must be active"
        assert abs(opt.last_grad_norm.item() - norm) <= 1e-5 * norm
        coef = min(1.0 / (norm + 1e-6), 1.0)
        ratios = []
        for p, w, gm in zip(ps, p0, mean):
            g = gm * coef
            wn, gn = w.norm(), g.norm()
            trust = tc * wn / (gn + wd * wn + eps)
            ratios.append(trust.item())
            want = w - lr * trust * (g + wd * w)
            assert torch.allclose(p.detach().double(), want, rtol=1e-5,
                                  atol=1e-6), \\
                (p.detach().double() - want).abs().max().item()
            # the averaged gradient is left unscaled
            assert torch.allclose(p.grad.double(), gm, rtol=1e-6, atol=1e-7)
        assert max(ratios) > 10 * min(ratios), ratios
        # both ranks share one GPU, so the parameters travel as host tensors
        bits = torch.cat([p.detach().reshape(-1) for p in ps]).cpu()
        both = hvd.allgather(bits.view(torch.int32), name="lars.param_bits")
        both = both.reshape(size, -1)
        assert bool((both == both[0]).all()), (both != both[0]).sum()
"""


@requires_gpu
def test_two_ranks_same_parameters():
    """Two ranks with different gradients take one clipped FusedLARS step
    through hvd.DistributedOptimizer: parameters match the definition on the
    mean gradient and are bitwise the same on both ranks, with no collective
    for the trust ratios."""
    run_workers(2, TWO_RANK_BODY,
                extra_env={"HOROVOD_ONESHOT_ALLREDUCE": "1"}, timeout=300)
