"""GPU tests (MI355X) for global-norm gradient clipping: the multi-tensor
norm / scale kernels (csrc/clip_kernels.hip), the grad_coef path of the
fused SGD / AdamW step kernels, and max_grad_norm= on FusedSGD / FusedAdamW.

References are torch.nn.utils.clip_grad_norm_ followed by the torch
optimizer, and an fp64 torch norm for the norm kernel itself.
"""
import warnings

import pytest
import torch

from tests.parallel_util import run_workers

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

SHAPES = [(33,), (128, 64), (7, 3, 3), (1024,)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["fp32", "bf16", "fp16"]

# tolerances of test_fused_sgd_matches_torch / test_fused_adamw_matches_torch
RTOL, ATOL = 1e-5, 1e-6

# AdamW is invariant to the gradient's scale but for eps, so a vanishing eps
# would hide a missing or wrong coefficient.  Clipped gradients are ~1e-2
# here; eps = 1e-3 makes a tenth of every update depend on the coefficient.
ADAMW_KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-3, weight_decay=0.05)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    yield


def _randn(shape, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).to(dtype)


def _grads(step, shapes=SHAPES):
    return [_randn(s, 1000 * step + i) for i, s in enumerate(shapes)]


def _param_pair(shapes=SHAPES, seed=5):
    ps = [_randn(s, seed * 100 + i).requires_grad_(True)
          for i, s in enumerate(shapes)]
    return ps, [p.detach().clone().requires_grad_(True) for p in ps]


# ---- norm kernel ----------------------------------------------------------

def _edge_list(dtype):
    """Empty, scalar, sub-vector, odd, just past a vector multiple, a view
    that is not 16-byte aligned, and one spanning many 8192-element chunks."""
    ts = [_randn((n,), 10 + n % 97, dtype) for n in (0, 1, 3, 33, 4097)]
    ts.append(_randn((1030,), 3, dtype)[1:])
    assert ts[-1].data_ptr() % 16 != 0
    ts.append(_randn((300000,), 4, dtype))
    return ts


def _many_list(dtype):
    """100 tensors of 5..40 elements: crosses the 48-descriptor capacity."""
    return [_randn((5 + (7 * i) % 36,), 200 + i, dtype) for i in range(100)]


def _ref_norm(ts):
    return torch.sqrt(sum((t.double() ** 2).sum() for t in ts))


def _torch_clip_norm(ts):
    """Norm returned by torch.nn.utils.clip_grad_norm_ for these gradients
    (max_norm so large that nothing is scaled)."""
    ps = []
    for t in ts:
        p = torch.empty_like(t).requires_grad_(True)
        p.grad = t.clone()
        ps.append(p)
    return torch.nn.utils.clip_grad_norm_(ps, 1e30)


def _norm_bound(ts, ref):
    torch_err = abs(_torch_clip_norm(ts).double().item() - ref) / ref
    return max(4 * torch_err, 4 * 2.0 ** -23), torch_err


@requires_gpu
@pytest.mark.parametrize("make", [_edge_list, _many_list],
                         ids=["edge_sizes", "100_tensors"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_norm_kernel_vs_fp64(dtype, make):
    from horovod_amd import _core
    ts = make(dtype)
    ref = _ref_norm(ts).item()
    out = _core.multi_tensor_grad_norm(ts, 1.0)
    assert out.dtype == torch.float32 and out.shape == (2,)
    norm, coef = out.tolist()
    err = abs(norm - ref) / ref
    bound, torch_err = _norm_bound(ts, ref)
    print(f"norm[{make.__name__},{dtype}]: native rel err {err:.3e}, "
          f"torch rel err {torch_err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    # coef = reciprocal(norm + 1e-6) * max_norm in fp32, clamped at 1
    want = (torch.tensor(norm, dtype=torch.float32) + 1e-6).reciprocal() * 1.0
    assert coef == min(want.item(), 1.0), (coef, want.item())


@requires_gpu
def test_norm_kernel_mixed_dtypes_one_call():
    """fp32, bf16 and fp16 gradients in one call: one launch per dtype, one
    norm over all of them."""
    from horovod_amd import _core
    ts = []
    for i in range(9):
        ts.append(_randn((1000 + 37 * i,), 300 + i, DTYPES[i % 3]))
    ref = _ref_norm(ts).item()
    norm = _core.multi_tensor_grad_norm(ts, 1.0)[0].item()
    assert abs(norm - ref) / ref <= 4 * 2.0 ** -23


@requires_gpu
def test_norm_kernel_empty_and_clamp():
    from horovod_amd import _core
    assert _core.multi_tensor_grad_norm([], 1.0).tolist() == [0.0, 1.0]
    empty = [torch.empty(0, device="cuda")]
    assert _core.multi_tensor_grad_norm(empty, 1.0).tolist() == [0.0, 1.0]
    small = [torch.full((16,), 0.25, device="cuda")]     # norm exactly 1
    assert _core.multi_tensor_grad_norm(small, 1e4).tolist() == [1.0, 1.0]


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_norm_kernel_deterministic(dtype):
    """No atomics: the same inputs give bitwise the same {norm, coef}."""
    from horovod_amd import _core
    ts = _edge_list(dtype) + _many_list(dtype)
    a = _core.multi_tensor_grad_norm(ts, 1.0)
    b = _core.multi_tensor_grad_norm(ts, 1.0)
    # the second call's workspace comes back from the caching allocator with
    # the first call's partials in it; a third gets garbage in between
    junk = torch.full((4096,), float("nan"), device="cuda")
    del junk
    c = _core.multi_tensor_grad_norm(ts, 1.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# ---- optimizers -----------------------------------------------------------

def _make(kind, params, **extra):
    from horovod_amd.ops import FusedAdamW, FusedSGD
    if kind == "adamw":
        return FusedAdamW(params, **ADAMW_KW, **extra)
    kw = dict(lr=0.1, weight_decay=0.01)
    if kind != "sgd_plain":
        kw["momentum"] = 0.9
    if kind == "sgd_nesterov":
        kw["nesterov"] = True
    return FusedSGD(params, **kw, **extra)


def _make_torch(kind, params):
    if kind == "adamw":
        return torch.optim.AdamW(params, **ADAMW_KW)
    kw = dict(lr=0.1, weight_decay=0.01)
    if kind != "sgd_plain":
        kw["momentum"] = 0.9
    if kind == "sgd_nesterov":
        kw["nesterov"] = True
    return torch.optim.SGD(params, **kw)


KINDS = ["adamw", "sgd_momentum", "sgd_nesterov", "sgd_plain"]


@requires_gpu
@pytest.mark.parametrize("kind", KINDS)
def test_inactive_clip_is_bitwise_noop(kind):
    """max_grad_norm above the norm: coef == 1.0 exactly, so the trajectory
    is bitwise the one of max_grad_norm=None."""
    ps_c, ps_n = _param_pair()
    oc = _make(kind, ps_c, max_grad_norm=1e4)
    on = _make(kind, ps_n)
    for step in range(6):
        for p, q, g in zip(ps_c, ps_n, _grads(step)):
            p.grad = g.clone()
            q.grad = g.clone()
        oc.step()
        on.step()
        for i, (p, q) in enumerate(zip(ps_c, ps_n)):
            assert torch.equal(p, q), (step, i, (p - q).abs().max().item())
    assert on.last_grad_norm is None
    assert 90 < oc.last_grad_norm.item() < 102


def _run_active(kind, shapes):
    ps_f, ps_r = _param_pair(shapes)
    of = _make(kind, ps_f, max_grad_norm=1.0)
    orr = _make_torch(kind, ps_r)
    for step in range(6):
        grads = _grads(step, shapes)
        for p, q, g in zip(ps_f, ps_r, grads):
            p.grad = g.clone()
            q.grad = g.clone()
        of.step()
        norm = torch.nn.utils.clip_grad_norm_(ps_r, 1.0)
        orr.step()
        assert norm.item() > 10, "clip must be active"
        assert of.last_grad_norm.dim() == 0
        assert torch.allclose(of.last_grad_norm, norm, rtol=1e-5, atol=0)
        for p, g in zip(ps_f, grads):
            assert torch.equal(p.grad, g), "step() must not scale p.grad"
        for i, (p, q) in enumerate(zip(ps_f, ps_r)):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
                (step, i, (p - q).abs().max().item())


@requires_gpu
@pytest.mark.parametrize("kind", KINDS)
def test_active_clip_matches_torch(kind):
    _run_active(kind, SHAPES)


@requires_gpu
def test_active_clip_adamw_60_params():
    """60 parameters: the norm and the step both take two launches and read
    one coefficient."""
    _run_active("adamw", [(17 + 5 * i,) for i in range(59)] + [(9000,)])


@requires_gpu
@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
def test_mixed_eligibility_bf16_param(kind):
    """A bf16 parameter among fp32 ones takes the eager update, but its
    gradient counts in the norm and is scaled by the same coefficient.

    The bf16 parameter is the small (33,) one: torch rounds that tensor's
    norm to bf16 before combining, and at 0.4% of the squared norm the
    rounding stays far below the fp32 tolerance.  bf16 tolerance: two ulp
    (2 * 2^-7 relative) on the parameter plus two ulp of the update's
    magnitude, which is at most 1e-2 (AdamW: lr * 1; SGD: lr * 0.05), so
    below 5e-4."""
    ps_f, ps_r = _param_pair()
    ps_f[0] = ps_f[0].detach().to(torch.bfloat16).requires_grad_(True)
    ps_r[0] = ps_f[0].detach().clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        of = _make(kind, ps_f, max_grad_norm=1.0)
        orr = _make_torch(kind, ps_r)
        grads = _grads(0)
        for p, q, g in zip(ps_f, ps_r, grads):
            p.grad = g.to(p.dtype).clone()
            q.grad = g.to(q.dtype).clone()
        of.step()
        norm = torch.nn.utils.clip_grad_norm_(ps_r, 1.0)
        orr.step()
    assert torch.allclose(of.last_grad_norm, norm.float(), rtol=1e-5, atol=0)
    assert torch.equal(ps_f[0].grad, grads[0].to(torch.bfloat16))
    assert ps_f[0].dtype == torch.bfloat16
    assert torch.allclose(ps_f[0].float(), ps_r[0].float(),
                          rtol=2.0 ** -6, atol=5e-4), \
        (ps_f[0].float() - ps_r[0].float()).abs().max().item()
    if kind == "sgd_momentum":
        # the buffer is coef * g + wd * p itself: an unclipped one is ~100x
        assert torch.allclose(of.state[ps_f[0]]["momentum_buffer"].float(),
                              orr.state[ps_r[0]]["momentum_buffer"].float(),
                              rtol=2.0 ** -6, atol=5e-4)
    for i, (p, q) in enumerate(zip(ps_f[1:], ps_r[1:])):
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), \
            (i, (p - q).abs().max().item())


@requires_gpu
@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_gradients_match_torch(kind, bad):
    ps_f, ps_r = _param_pair()
    of = _make(kind, ps_f, max_grad_norm=1.0)
    orr = _make_torch(kind, ps_r)
    grads = _grads(0)
    grads[1][5, 7] = float(bad)
    for p, q, g in zip(ps_f, ps_r, grads):
        p.grad = g.clone()
        q.grad = g.clone()
    of.step()
    torch.nn.utils.clip_grad_norm_(ps_r, 1.0)
    orr.step()
    for p, q in zip(ps_f, ps_r):
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL, equal_nan=True)
    if bad == "nan":
        # NaN norm -> NaN coefficient -> every element of every parameter
        assert all(torch.isnan(p).all() for p in ps_f)
        assert torch.isnan(of.last_grad_norm)
    else:
        # infinite norm -> coefficient 0; inf * 0 is NaN at that element only
        nan = torch.cat([torch.isnan(p).flatten() for p in ps_f])
        assert nan.sum().item() == 1 and torch.isnan(ps_f[1][5, 7])
        assert torch.isinf(of.last_grad_norm)


# ---- functional clip_grad_norm_ -------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_functional_clip_matches_torch(dtype):
    from horovod_amd.ops import clip_grad_norm_
    # the four small shapes, a view that is not 16-byte aligned, and a
    # tensor of several chunks
    grads = [g.to(dtype) for g in _grads(0)]
    grads += [_randn((1030,), 8, dtype)[1:], _randn((20000,), 9, dtype)]
    ps_f = [torch.empty_like(g).requires_grad_(True) for g in grads]
    ps_r = [torch.empty_like(g).requires_grad_(True) for g in grads]
    for p, q, g in zip(ps_f, ps_r, grads):
        p.grad = g.clone() if g.data_ptr() % 16 == 0 else g
        q.grad = g.clone()
    assert ps_f[4].grad.data_ptr() % 16 != 0
    grads = [g.clone() for g in grads]
    ref = _ref_norm(grads).item()
    bound, torch_err = _norm_bound(grads, ref)
    norm = clip_grad_norm_(ps_f, 1.0)
    norm_t = torch.nn.utils.clip_grad_norm_(ps_r, 1.0)
    err = abs(norm.item() - ref) / ref
    print(f"functional[{dtype}]: native rel err {err:.3e}, torch rel err "
          f"{torch_err:.3e}, bound {bound:.3e}")
    assert norm.dim() == 0 and err <= bound, (err, bound)
    # 16-bit gradients: torch rounds its norm and its coefficient to the
    # dtype (half an ulp = eps / 2 each), and the two rounded products can
    # then differ by one more ulp (eps)
    rtol = 1e-6 if dtype == torch.float32 else 2 * torch.finfo(dtype).eps
    # clipped fp16 gradients below 6.1e-5 are subnormal, on a grid of 2^-24
    # whatever their size: the same two roundings are two grid steps there
    atol = 2 * 2.0 ** -24 if dtype == torch.float16 else 0
    assert norm_t.dim() == 0
    for p, q in zip(ps_f, ps_r):
        assert p.grad.dtype == dtype
        assert torch.allclose(p.grad.float(), q.grad.float(), rtol=rtol,
                              atol=atol), \
            (p.grad.float() - q.grad.float()).abs().max().item()


@requires_gpu
def test_functional_clip_below_max_norm_leaves_grads():
    from horovod_amd.ops import clip_grad_norm_
    ps, _ = _param_pair()
    grads = _grads(0)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    norm = clip_grad_norm_(ps, 1e4)
    assert abs(norm.item() - _ref_norm(grads).item()) < 1e-3
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad, g)


@requires_gpu
def test_scale_kernel_nan_coef_is_not_skipped():
    from horovod_amd import _core
    t = torch.ones(100, device="cuda")
    _core.multi_tensor_scale_([t], torch.full((1,), float("nan"),
                                              device="cuda"))
    assert torch.isnan(t).all()


# ---- two ranks ------------------------------------------------------------

TWO_RANK_BODY = """
        from horovod_amd import _core
        from horovod_amd.ops import FusedAdamW
        torch.cuda.set_device(hvd.local_rank() % torch.cuda.device_count())
        dev = torch.device("cuda",
                           hvd.local_rank() % torch.cuda.device_count())
        shapes = [(33,), (128, 64), (7, 3, 3), (1024,)]
        kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-3, weight_decay=0.05)

        def randn(seed):
            g = torch.Generator().manual_seed(seed)
            return [torch.randn(s, generator=g).to(dev) for s in shapes]

        ps = [p.requires_grad_(True) for p in randn(1)]   # same on all ranks
        ps_ref = [p.detach().clone().requires_grad_(True) for p in ps]
        per_rank = [randn(50 + r) for r in range(size)]
        opt = hvd.DistributedOptimizer(
            FusedAdamW(ps, max_grad_norm=1.0, **kw),
            named_parameters=[(f"p{i}", p) for i, p in enumerate(ps)])
        assert all(g["max_grad_norm"] == 1.0 for g in opt.param_groups)
        for p, g in zip(ps, per_rank[rank]):
            p.grad = g.clone()
        opt.step()
        torch.cuda.synchronize()
        assert not _core.rccl_used(), "small gradients must stay one-shot"

        mean = [sum(gs) / size for gs in zip(*per_rank)]
        for q, g in zip(ps_ref, mean):
            q.grad = g.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(ps_ref, 1.0)
        torch.optim.AdamW(ps_ref, **kw).step()
        assert ref_norm.item() > 10, "clip must be active"
        assert torch.allclose(opt.last_grad_norm, ref_norm, rtol=1e-5)
        for p, q, g in zip(ps, ps_ref, mean):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), \\
                (p - q).abs().max().item()
            # the averaged gradient is left unscaled
            assert torch.allclose(p.grad, g, rtol=1e-6, atol=1e-7)
        # both ranks share one GPU, so the norms travel as host tensors
        bits = opt.last_grad_norm.reshape(1).cpu().view(torch.int32)
        both = hvd.allgather(bits, name="clip.norm_bits")
        assert both.numel() == size and bool((both == both[0]).all()), both
"""


@requires_gpu
def test_two_ranks_clip_same_coefficient():
    """Two ranks with different gradients take one clipped FusedAdamW step
    through hvd.DistributedOptimizer: parameters match clip + AdamW on the
    mean gradient, and the norm is bitwise the same on both ranks."""
    run_workers(2, TWO_RANK_BODY,
                extra_env={"HOROVOD_ONESHOT_ALLREDUCE": "1"}, timeout=300)
