"""GPU tests (MI355X) of the master-weight kernels: _core.fused_sgd_step /
fused_adamw_step / fused_lamb_step with model_params=, and the optimizers
with master_weights=True on CUDA fp16/bf16 parameters.

Inputs are the edge list and the 100-tensor capacity list of
test_gpu_fused_steps.py with the gradients rounded to fp16 / bf16 and a
2-byte model parameter next to every fp32 parameter (the master), plus

  * a tuple whose 2-byte rows start 4 elements into their storage (8-byte
    aligned) while the fp32 rows are 16-byte aligned: the 16-byte loop must
    not run, every row has to be aligned for it;
  * a 40 000-element tuple: SGD and AdamW give a tensor 16 blocks of 256
    lanes, 8 elements per lane, so one grid-stride sweep covers 32 768;
  * the capacity list with fp16 and bf16 alternating, 50 tensors each, so
    both per-dtype batches flush twice.

SGD and AdamW: the per-element function is the one of the fp32 kernels and
widening a 2-byte gradient is exact, so masters and moments must equal,
bit for bit, the fp32 kernel run on grads.float().  LAMB's sums run in
another order (8 elements per lane), so it is held to the fp64 definition
(RefLamb) at the project's rtol=1e-5, atol=1e-6 like the fp32 kernels, trust
ratios included.  The model parameter must always be the rounded master.
"""
import warnings

import pytest
import torch

from tests.test_gpu_fused_steps import (ADAMW, ADAMW_STEPS, ATOL, RTOL,
                                        SGD_VARIANTS, _randn, _tuple,
                                        edge_tuples, many_tuples,
                                        requires_gpu)
from tests.test_gpu_lamb import HYPER, _ref_direct

pytestmark = pytest.mark.gpu

LOW = {"fp16": torch.float16, "bf16": torch.bfloat16}
SWEEP = 16 * 256 * 8          # elements of one grid-stride sweep, 8 per lane


@pytest.fixture(scope="module", autouse=True)
def _device():
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    yield


# ---- inputs ------------------------------------------------------------------

def _at_offset(x, dtype=None, offset=None):
    """A copy of x in `dtype` that starts `offset` elements into its storage
    (default: where x starts in its own, so alignment classes carry over)."""
    offset = x.storage_offset() if offset is None else offset
    buf = torch.empty(x.numel() + offset, dtype=dtype or x.dtype,
                      device=x.device)
    out = buf[offset:]
    out.copy_(x)
    return out


def _base_tuples(which):
    if which == "edge":
        ts = edge_tuples()
        ts.append(_tuple(1029, 3))               # its 2-byte rows: offset 4
        ts.append(_tuple(40000, 5))
        assert ts[-1][0].numel() > SWEEP
        return ts, {len(ts) - 2: 4}
    return many_tuples(), {}


def _dtypes(which, low, n):
    if which == "capacity_mixed":
        return [(torch.float16, torch.bfloat16)[i % 2] for i in range(n)]
    return [LOW[low]] * n


CASES = [("edge", "fp16"), ("edge", "bf16"), ("capacity", "fp16"),
         ("capacity", "bf16"), ("capacity_mixed", "both")]
CASE_IDS = [f"{w}-{d}" for w, d in CASES]


class Inputs:
    """fp32 tuples (p, g, m, v) with g already rounded to the 2-byte dtype,
    and the matching master-weight tuples (p, g_lp, m, v, model)."""

    def __init__(self, which, low):
        base, lp_offsets = _base_tuples(
            "capacity" if which.startswith("capacity") else which)
        dts = _dtypes(which, low, len(base))
        self.fp32, self.lp, self.model = [], [], []
        for i, (t, dt) in enumerate(zip(base, dts)):
            off = lp_offsets.get(i)
            g_lp = _at_offset(t[1], dt, off)
            self.lp.append(g_lp)
            # what the kernel must overwrite
            self.model.append(_at_offset(torch.full_like(t[0], 7.0), dt, off))
            self.fp32.append([t[0], _at_offset(g_lp, torch.float32,
                                               t[1].storage_offset()),
                              t[2], t[3]])
        for i, off in lp_offsets.items():
            assert self.lp[i].data_ptr() % 16 == 8
            assert self.model[i].data_ptr() % 16 == 8
            assert all(x.data_ptr() % 16 == 0 for x in self.fp32[i])

    def fresh(self):
        """-> (fp32 tuples, master-weight tuples), new copies of both."""
        a = [[_at_offset(x) for x in t] for t in self.fp32]
        b = [[_at_offset(t[0]), _at_offset(g), _at_offset(t[2]),
              _at_offset(t[3]), _at_offset(q)]
             for t, g, q in zip(self.fp32, self.lp, self.model)]
        return a, b


_inputs_cache = {}


def _inputs(which, low):
    key = (which, low)
    if key not in _inputs_cache:
        _inputs_cache[key] = Inputs(which, low)
    return _inputs_cache[key]


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _model_is_rounded_master(mw):
    for i, t in enumerate(mw):
        assert _same_bits(t[4], t[0].to(t[4].dtype)), (i, "model != master")


# ---- SGD and AdamW: bitwise the fp32 kernel on grads.float() -----------------

def _sgd(tuples, kw, coef, master):
    from horovod_amd import _core
    _core.fused_sgd_step([t[0] for t in tuples], [t[1] for t in tuples],
                         [t[2] for t in tuples] if kw["momentum"] else [],
                         kw["lr"], kw["momentum"], kw["weight_decay"],
                         kw["dampening"], kw["nesterov"], coef,
                         [t[4] for t in tuples] if master else None)


def _adamw(tuples, step, coef, master):
    from horovod_amd import _core
    _core.fused_adamw_step([t[0] for t in tuples], [t[1] for t in tuples],
                           [t[2] for t in tuples], [t[3] for t in tuples],
                           ADAMW["lr"], ADAMW["beta1"], ADAMW["beta2"],
                           ADAMW["eps"], ADAMW["weight_decay"], step, coef,
                           [t[4] for t in tuples] if master else None)


def _check_bitwise(inputs, call):
    coef = torch.full((1,), 0.25, device="cuda")
    for c in (None, coef):
        ref, mw = inputs.fresh()
        call(ref, c, False)
        call(mw, c, True)
        for i, (r, t, g) in enumerate(zip(ref, mw, inputs.lp)):
            assert _same_bits(t[1], g), (i, "gradients are only read")
            for k in (0, 2, 3):
                assert _same_bits(t[k], r[k]), \
                    (i, k, c is not None, (t[k] - r[k]).abs().max().item())
        _model_is_rounded_master(mw)
    # the step did something, and not only to the master
    assert not torch.equal(mw[-1][0], inputs.fp32[-1][0])
    assert not torch.equal(mw[-1][4], inputs.model[-1])


@requires_gpu
@pytest.mark.parametrize("which,low", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("variant", list(SGD_VARIANTS))
def test_sgd_master_kernel_bitwise_fp32_kernel(variant, which, low):
    kw = SGD_VARIANTS[variant]
    _check_bitwise(_inputs(which, low),
                   lambda tuples, c, master: _sgd(tuples, kw, c, master))


@requires_gpu
@pytest.mark.parametrize("which,low", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("step", ADAMW_STEPS)
def test_adamw_master_kernel_bitwise_fp32_kernel(step, which, low):
    _check_bitwise(_inputs(which, low),
                   lambda tuples, c, master: _adamw(tuples, step, c, master))


# ---- LAMB: the fp64 definition -------------------------------------------------

def _lamb(tuples, weight_decay, coef=None):
    from horovod_amd import _core
    return _core.fused_lamb_step(
        [t[0] for t in tuples], [t[1] for t in tuples],
        [t[2] for t in tuples], [t[3] for t in tuples],
        weight_decay=weight_decay, grad_coef=coef,
        model_params=[t[4] for t in tuples], **HYPER)


def _close(got, want, where):
    got = got.double()
    assert torch.allclose(got, want, rtol=RTOL, atol=ATOL), \
        (where, (got - want).abs().max().item())


@requires_gpu
@pytest.mark.parametrize("which,low", CASES, ids=CASE_IDS)
def test_lamb_master_kernel_vs_fp64(which, low):
    inputs = _inputs(which, low)
    before, mw = inputs.fresh()
    ref = _ref_direct(before, 0.01)
    trust = _lamb(mw, 0.01)
    assert trust.dtype == torch.float32 and trust.shape == (len(mw),)
    for i, (t, g) in enumerate(zip(mw, inputs.lp)):
        assert _same_bits(t[1], g), (i, "gradients are only read")
        _close(t[0], ref.p[i], (i, "p"))
        _close(t[2], ref.m[i], (i, "m"))
        _close(t[3], ref.v[i], (i, "v"))
    _close(trust.cpu(), torch.tensor(ref.trust, dtype=torch.float64), "trust")
    _model_is_rounded_master(mw)
    assert min(ref.trust) < 0.5 and max(ref.trust) > 2, ref.trust
    assert not torch.equal(mw[-1][4], inputs.model[-1])
    # identical inputs, identical bits
    _, again = inputs.fresh()
    trust2 = _lamb(again, 0.01)
    assert _same_bits(trust, trust2)
    for i, (a, b) in enumerate(zip(mw, again)):
        for k in (0, 2, 3, 4):
            assert _same_bits(a[k], b[k]), (i, k)


@requires_gpu
def test_lamb_master_kernel_with_coef_vs_fp64():
    """grad_coef on the master-weight path: the definition on gradients
    scaled beforehand (0.25 is a power of two, so that scaling is exact)."""
    inputs = _inputs("edge", "bf16")
    before, mw = inputs.fresh()
    for t in before:
        t[1] = t[1] * 0.25
    ref = _ref_direct(before, 0.01)
    trust = _lamb(mw, 0.01, torch.full((1,), 0.25, device="cuda"))
    for i, t in enumerate(mw):
        _close(t[0], ref.p[i], (i, "p"))
        _close(t[2], ref.m[i], (i, "m"))
        _close(t[3], ref.v[i], (i, "v"))
    _close(trust.cpu(), torch.tensor(ref.trust, dtype=torch.float64), "trust")
    _model_is_rounded_master(mw)


# ---- rounding ------------------------------------------------------------------

def _from_bits(words):
    """fp32 tensor (CPU) of the given 32-bit words."""
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words],
                        dtype=torch.int32).view(torch.float32)


BF16_WORDS = [(0x3F808000, 0x3F80),   # tie above an even mantissa: down
              (0x3F818000, 0x3F82),   # tie above an odd mantissa: up
              (0x7F7FFFFF, 0x7F80),   # largest fp32: rounds to infinity
              (0x80000000, 0x8000),   # -0.0
              (0x00000001, 0x0000)]   # smallest subnormal
FP16_WORDS = [(0x3F801000, 0x3C00),   # tie above an even mantissa
              (0x3F803000, 0x3C02),   # tie above an odd mantissa
              (0x477FE000, 0x7BFF),   # 65504, the largest fp16
              (0x477FEFFF, 0x7BFF),   # just under the tie to 65536
              (0x477FF000, 0x7C00),   # that tie: even is 65536 = infinity
              (0x38800000, 0x0400),   # smallest normal
              (0x33800000, 0x0001),   # smallest subnormal, 2^-24
              (0x33000000, 0x0000),   # 2^-25: tie between 0 and 2^-24
              (0x33000001, 0x0001),   # just above it
              (0x33C00000, 0x0002),   # 1.5 * 2^-24: tie, even is 2
              (0x387FC000, 0x03FF),   # largest subnormal
              (0x387FE000, 0x0400),   # tie to the smallest normal
              (0x80000000, 0x8000),
              (0x00000001, 0x0000)]


@requires_gpu
@pytest.mark.parametrize("low,table", [("bf16", BF16_WORDS),
                                       ("fp16", FP16_WORDS)])
def test_model_parameter_is_rounded_to_nearest_even(low, table):
    """lr = weight_decay = momentum = 0 and a zero gradient leave the master
    as it is; the model parameter must get it rounded as the CPU rounds.
    19 or 38+ elements: the 16-byte loop and the tail both convert."""
    from horovod_amd import _core
    dtype = LOW[low]
    words = [w for w, _ in table] * 3 + [w for w, _ in table][:3]
    want = [h for _, h in table] * 3 + [h for _, h in table][:3]
    cpu_master = _from_bits(words)
    assert len(words) % 8 != 0 and len(words) > 8
    master = cpu_master.cuda()
    model = torch.full((len(words),), 7.0, dtype=dtype, device="cuda")
    grad = torch.zeros(len(words), dtype=dtype, device="cuda")
    _core.fused_sgd_step([master], [grad], [], 0.0, 0.0, 0.0, 0.0, False,
                         None, [model])
    assert torch.equal(_bits(master.cpu()), _bits(cpu_master))
    got = _bits(model.cpu()).tolist()
    cpu = _bits(cpu_master.to(dtype)).tolist()
    want = [h - (1 << 16) if h >= 1 << 15 else h for h in want]
    assert got == cpu, [(hex(w), g, c) for w, g, c in zip(words, got, cpu)
                        if g != c]
    assert got == want


# ---- rejection -----------------------------------------------------------------

def _steps():
    from horovod_amd import _core
    return {
        "sgd": lambda p, g, m, v, q: _core.fused_sgd_step(
            p, g, m, 0.1, 0.9, 0.01, 0.0, False, None, q),
        "adamw": lambda p, g, m, v, q: _core.fused_adamw_step(
            p, g, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.05, 3, None, q),
        "lamb": lambda p, g, m, v, q: _core.fused_lamb_step(
            p, g, m, v, 1e-2, 0.9, 0.95, 1e-6, 0.01, 3, True, True, None, q),
    }


@requires_gpu
@pytest.mark.parametrize("op", ["sgd", "adamw", "lamb"])
def test_master_kernels_reject_bad_inputs(op):
    call = _steps()[op]
    p, g, m, v = _tuple(16, 1)
    ok = _tuple(16, 21)                          # a good tuple ahead of it
    keep, keep_ok = p.clone(), ok[0].clone()
    bf, half = torch.bfloat16, torch.float16

    def run(p_, g_, m_, v_, q_, first=True):
        lead = [[ok[0]], [ok[1].to(bf)], [ok[2]], [ok[3]], [ok[0].to(bf)]]
        if not first:
            lead = [[] for _ in lead]
        call(*[a + b for a, b in zip(lead, (p_, g_, m_, v_, q_))])

    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        run([p], [g.to(bf)], [m], [v], [p.clone()])        # fp32 model
    with pytest.raises(RuntimeError, match="dtype"):
        run([p], [g.to(half)], [m], [v], [p.to(bf)])       # grad != model
    with pytest.raises(RuntimeError, match="dtype"):
        run([p], [g], [m], [v], [p.to(bf)])                # fp32 gradient
    with pytest.raises(RuntimeError, match="fp32 masters"):
        run([p.to(bf)], [g.to(bf)], [m], [v], [p.to(bf)])  # bf16 masters
    with pytest.raises(RuntimeError, match="fp32 masters"):
        run([p], [g.to(bf)], [m.to(bf)], [v.to(bf)], [p.to(bf)])
    with pytest.raises(RuntimeError, match="as many model_params"):
        run([p], [g.to(bf)], [m], [v], [])                 # length
    with pytest.raises(RuntimeError, match="size"):
        run([p], [g.to(bf)], [m], [v], [p.to(bf)[:7]])     # size
    with pytest.raises(RuntimeError, match="GPU"):
        run([p], [g.to(bf)], [m], [v], [p.to(bf).cpu()])
    # nothing was launched, not even for the good tuple ahead
    assert _same_bits(p, keep) and _same_bits(ok[0], keep_ok)
    run([], [], [], [], [], first=False)                   # empty: a no-op


# ---- optimizer level -----------------------------------------------------------

SHAPES = [(33,), (128, 24), (7, 3, 3), (1029,)]


def _exact_grad(shape, seed):
    """Multiples of 1/8 up to 4: exact in bf16, and the squares of all 4197
    elements sum exactly in fp32 in any order (at most 4197 * 1024 < 2^24
    units of 1/64).  The clip kernel's summation order depends on the
    gradient dtype (8 bf16 or 4 fp32 elements per lane), so only such
    gradients have one norm whatever their dtype."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 33, shape, generator=g).float() / 8).cuda()


@requires_gpu
def test_fused_adamw_master_weights_follows_fp32_fused_adamw():
    from horovod_amd.ops import FusedAdamW
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05,
              max_grad_norm=1.0)
    ps = [_randn(s, 70 + i).bfloat16().requires_grad_(True)
          for i, s in enumerate(SHAPES)]
    qs = [p.detach().float().requires_grad_(True) for p in ps]
    start = [p.detach().clone() for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no eager update anywhere
        opt = FusedAdamW(ps, master_weights=True, **kw)
        ref = FusedAdamW(qs, **kw)
        for step in range(4):
            for i, (p, q) in enumerate(zip(ps, qs)):
                g = _exact_grad(p.shape, 300 + 10 * step + i)
                p.grad = g.bfloat16()
                q.grad = p.grad.float()
                assert torch.equal(q.grad, g)
            opt.step()
            ref.step()
            assert opt.last_grad_norm.item() > 50, "clip must be active"
            assert torch.equal(opt.last_grad_norm, ref.last_grad_norm)
            for i, (p, q) in enumerate(zip(ps, qs)):
                st = opt.state[p]
                assert st["master_param"].dtype == torch.float32
                assert _same_bits(st["master_param"], q.detach()), (step, i)
                assert _same_bits(st["exp_avg"], ref.state[q]["exp_avg"])
                assert _same_bits(st["exp_avg_sq"],
                                  ref.state[q]["exp_avg_sq"])
                assert _same_bits(p.detach(), q.detach().bfloat16())
                assert _same_bits(p.grad, q.grad.bfloat16())
    assert all(not torch.equal(p.detach(), s) for p, s in zip(ps, start))


@requires_gpu
@pytest.mark.parametrize("name", ["FusedSGD", "FusedLAMB"])
def test_mixed_group_takes_both_kernels_without_warning(name):
    """fp32, fp16 and bf16 parameters in one master_weights group: none takes
    the eager update, only the 2-byte ones get a master, and each stays the
    rounded master."""
    import horovod_amd.ops as ops
    kw = dict(lr=1e-2, weight_decay=0.01, master_weights=True)
    if name == "FusedSGD":
        kw["momentum"] = 0.9
    dts = [torch.float32, torch.float16, torch.bfloat16, torch.float32]
    ps = [_randn(s, 80 + i).to(dt).requires_grad_(True)
          for i, (s, dt) in enumerate(zip(SHAPES, dts))]
    start = [p.detach().clone() for p in ps]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt = getattr(ops, name)(ps, **kw)
        for step in range(2):
            for i, p in enumerate(ps):
                p.grad = _randn(p.shape, 90 + 10 * step + i).to(p.dtype)
            opt.step()
    for p, s in zip(ps, start):
        st = opt.state[p]
        assert not torch.equal(p.detach(), s)
        moments = [st[k] for k in ("momentum_buffer", "exp_avg", "exp_avg_sq")
                   if k in st]
        assert moments and all(x.dtype == torch.float32 for x in moments)
        if p.dtype == torch.float32:
            assert "master_param" not in st
        else:
            assert st["master_param"].dtype == torch.float32
            assert _same_bits(p.detach(), st["master_param"].to(p.dtype))
