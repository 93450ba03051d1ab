"""Native SyncBatchNorm path (csrc/syncbn_kernels.hip) on one MI355X.

Single-process tests call _SyncBatchNormFn.apply directly (the module falls
back to plain BatchNorm at world size 1) and compare against
torch.nn.functional.batch_norm(training=True) run in fp64 on a CPU copy of
the same, already dtype-rounded, input.  The two-rank test shares device 0
between two processes over the one-shot allreduce, as test_gpu_oneshot.py
does.

Tolerances are the project's own from test_fused_bn_relu_matches_torch:
fp32 2e-4; fp16/bf16 outputs and dx 5e-2; parameter grads 1e-2;
running_mean 1e-4; running_var 1e-3.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.parallel_util import run_workers

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

EPS = 1e-5
MOMENTUM = 0.1


def _tol(dtype):
    return 2e-4 if dtype == torch.float32 else 5e-2


@pytest.fixture(scope="module")
def hvd():
    import horovod_amd.torch as hvd
    hvd.init()
    torch.cuda.set_device(0)
    yield hvd
    # process-level shutdown handled by atexit


def _close(got, ref, tol, what):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bound = tol + tol * ref.abs()
    assert bool((err <= bound).all()), \
        f"{what}: max err {err.max().item():.3e}, " \
        f"{int((err > bound).sum())}/{err.numel()} outside tol {tol}"


def _make_input(shape, dtype, channels_last, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * scale + shift).to(dtype)
    x = x.cuda()
    if channels_last:
        fmt = torch.channels_last if x.dim() == 4 else torch.channels_last_3d
        x = x.contiguous(memory_format=fmt)
    return x


def _run_case(hvd, shape, dtype, channels_last=False, affine=True,
              running=True, param_dtype=None, grad="randn", seed=0):
    """fwd+bwd through the native path vs the fp64 reference."""
    from horovod_amd.torch.sync_batch_norm import (_SyncBatchNormFn,
                                                   native_eligible)
    tol = _tol(dtype)
    param_dtype = param_dtype or dtype
    C = shape[1]
    g = torch.Generator().manual_seed(1000 + seed)
    x = _make_input(shape, dtype, channels_last, seed=seed).requires_grad_(True)
    assert native_eligible(x)
    w = b = None
    if affine:
        w = (torch.rand(C, generator=g) + 0.5).to(param_dtype).cuda() \
            .requires_grad_(True)
        b = torch.randn(C, generator=g).to(param_dtype).cuda() \
            .requires_grad_(True)
    rm = rv = None
    if running:
        rm = torch.full((C,), 0.5, device="cuda")
        rv = torch.full((C,), 2.0, device="cuda")

    out = _SyncBatchNormFn.apply(x, w, b, rm, rv, EPS, MOMENTUM,
                                 hvd.global_process_set)
    assert out.dtype == dtype and out.shape == x.shape
    assert out.stride() == x.stride(), "output must keep the input's layout"
    if channels_last:
        fmt = torch.channels_last if x.dim() == 4 else torch.channels_last_3d
        assert out.is_contiguous(memory_format=fmt)

    if grad == "randn":
        dy = torch.randn(*shape, generator=g).to(dtype).cuda()
        if channels_last:
            dy = dy.contiguous(memory_format=fmt)
    elif grad == "transposed":
        # same logical shape, non-contiguous memory
        perm = list(shape)
        perm[-1], perm[-2] = perm[-2], perm[-1]
        dy = torch.randn(*perm, generator=g).to(dtype).cuda() \
            .transpose(-1, -2)
        assert not dy.is_contiguous()
    if grad == "sum":
        out.sum().backward()  # autograd hands over an expanded grad
        dy = torch.ones(shape, dtype=dtype)
    else:
        out.backward(dy)
    torch.cuda.synchronize()

    # fp64 reference on the same rounded values
    xr = x.detach().double().cpu().contiguous().requires_grad_(True)
    wr = w.detach().double().cpu().requires_grad_(True) if affine else None
    br = b.detach().double().cpu().requires_grad_(True) if affine else None
    rmr = torch.full((C,), 0.5, dtype=torch.float64) if running else None
    rvr = torch.full((C,), 2.0, dtype=torch.float64) if running else None
    yr = F.batch_norm(xr, rmr, rvr, wr, br, True, MOMENTUM, EPS)
    yr.backward(dy.detach().double().cpu())

    tag = f"{shape} {dtype} cl={channels_last}"
    _close(out, yr.detach(), tol, f"out {tag}")
    _close(x.grad, xr.grad, tol, f"dx {tag}")
    assert x.grad.stride() == x.stride()
    if affine:
        assert w.grad.dtype == w.dtype and b.grad.dtype == b.dtype
        _close(w.grad, wr.grad, 1e-2, f"grad_weight {tag}")
        _close(b.grad, br.grad, 1e-2, f"grad_bias {tag}")
    if running:
        _close(rm, rmr, 1e-4, f"running_mean {tag}")
        _close(rv, rvr, 1e-3, f"running_var {tag}")


PLANAR_SHAPES = [
    (4, 3, 5, 7),      # C % 8 != 0, odd L: 2-byte rows are misaligned
    (5, 10),           # 2-D, L = 1
    (3, 16, 1000),     # 3-D
    (2, 1, 1, 1),      # C = 1, count 2
    (8, 32, 56, 56),   # several blocks per channel, grid-stride
]


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=str)
def test_planar(hvd, shape, dtype):
    _run_case(hvd, shape, dtype)


@requires_gpu
@pytest.mark.parametrize("shape,dtype", [
    ((4, 64, 7, 7), torch.float32),
    ((4, 64, 7, 7), torch.bfloat16),
    ((3, 12, 5, 5), torch.float32),     # C % 8 != 0
    ((3, 12, 5, 5), torch.bfloat16),
    ((8, 2048, 7, 7), torch.float32),   # wide C
    ((5, 24, 9, 9), torch.float32),     # C/8 not a power of two
    ((64, 512, 4, 4), torch.bfloat16),  # several vectors per thread
    ((2, 16, 3, 4, 5), torch.float32),  # channels_last_3d
], ids=str)
def test_channels_last(hvd, shape, dtype):
    _run_case(hvd, shape, dtype, channels_last=True)


@requires_gpu
def test_planar_fp16_and_8_byte_runs(hvd):
    """fp16, and L = 196: 2-byte rows that are 8-B but not 16-B aligned."""
    _run_case(hvd, (4, 3, 5, 7), torch.float16)
    _run_case(hvd, (3, 5, 14, 14), torch.bfloat16)
    _run_case(hvd, (3, 5, 14, 14), torch.float16)
    _run_case(hvd, (3, 5, 3, 6), torch.float32)


@requires_gpu
@pytest.mark.parametrize("channels_last", [False, True],
                         ids=["planar", "channels_last"])
def test_options(hvd, channels_last):
    shape = (4, 16, 6, 5)
    for dtype in (torch.float32, torch.bfloat16):
        _run_case(hvd, shape, dtype, channels_last, affine=False)
        _run_case(hvd, shape, dtype, channels_last, running=False)
        _run_case(hvd, shape, dtype, channels_last, grad="sum")
        _run_case(hvd, shape, dtype, channels_last, grad="transposed")
    # autocast-style: fp32 parameters with a bf16 activation
    _run_case(hvd, shape, torch.bfloat16, channels_last,
              param_dtype=torch.float32)


@requires_gpu
def test_bf16_running_stats_fallback(hvd):
    """Non-fp32 running stats take the ATen update.  Tolerance: the update
    rounds to bf16 (2^-8 relative) twice, on values of at most 2."""
    from horovod_amd.torch.sync_batch_norm import _SyncBatchNormFn
    x = _make_input((4, 6, 5, 7), torch.bfloat16, False, seed=3)
    rm = torch.full((6,), 0.5, device="cuda", dtype=torch.bfloat16)
    rv = torch.full((6,), 2.0, device="cuda", dtype=torch.bfloat16)
    _SyncBatchNormFn.apply(x, None, None, rm, rv, EPS, MOMENTUM,
                           hvd.global_process_set)
    rmr = torch.full((6,), 0.5, dtype=torch.float64)
    rvr = torch.full((6,), 2.0, dtype=torch.float64)
    F.batch_norm(x.double().cpu(), rmr, rvr, None, None, True, MOMENTUM, EPS)
    _close(rm, rmr, 2e-2, "bf16 running_mean")
    _close(rv, rvr, 2e-2, "bf16 running_var")


@requires_gpu
def test_half_precision_statistics_are_fp32(hvd):
    """bf16 input with mean 3.0 and std 0.25: statistics carried in bf16
    collapse the variance to 0 or 0.0625 (true value ~0.06) and miss the
    fp64 reference by up to 365; fp32 statistics leave only the output
    rounding (max error 0.014 in a CPU model of the maths).  Every element
    must be inside the bf16 tolerance."""
    from horovod_amd.torch.sync_batch_norm import (_SyncBatchNormFn,
                                                   native_eligible)
    x = _make_input((4, 16, 9, 7), torch.bfloat16, False, seed=0,
                    scale=0.25, shift=3.0)
    assert native_eligible(x)
    out = _SyncBatchNormFn.apply(x, None, None, None, None, EPS, MOMENTUM,
                                 hvd.global_process_set)
    ref = F.batch_norm(x.double().cpu(), None, None, None, None, True,
                       MOMENTUM, EPS)
    err = (out.double().cpu() - ref).abs()
    print(f"bf16 offset-input max err {err.max().item():.4f}")
    _close(out, ref, 5e-2, "bf16 offset input")


@requires_gpu
def test_env_switch_takes_composite_path():
    """HOROVOD_SYNC_BN_NATIVE=0 keeps GPU tensors on the composite code,
    which still matches in fp32."""
    run_workers(1, """
        import torch.nn.functional as F
        from horovod_amd.torch.sync_batch_norm import (_SyncBatchNormFn,
                                                       native_eligible)
        torch.cuda.set_device(0)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(4, 6, 5, 7, generator=g).cuda().requires_grad_(True)
        assert not native_eligible(x)
        w = (torch.rand(6, generator=g) + 0.5).cuda()
        b = torch.randn(6, generator=g).cuda()
        rm = torch.zeros(6, device="cuda")
        rv = torch.ones(6, device="cuda")
        out = _SyncBatchNormFn.apply(x, w, b, rm, rv, 1e-5, 0.1,
                                     hvd.global_process_set)
        dy = torch.randn(4, 6, 5, 7, generator=g)
        out.backward(dy.cuda())
        xr = x.detach().double().cpu().requires_grad_(True)
        rmr = torch.zeros(6, dtype=torch.float64)
        rvr = torch.ones(6, dtype=torch.float64)
        yr = F.batch_norm(xr, rmr, rvr, w.double().cpu(), b.double().cpu(),
                          True, 0.1, 1e-5)
        yr.backward(dy.double())
        def close(a, r, tol):
            return torch.allclose(a.detach().double().cpu(), r, rtol=tol,
                                  atol=tol)
        assert close(out, yr.detach(), 2e-4)
        assert close(x.grad, xr.grad, 2e-4)
        assert close(rm, rmr, 1e-4) and close(rv, rvr, 1e-3)
    """, extra_env={"HOROVOD_SYNC_BN_NATIVE": "0"}, timeout=300)


ONESHOT_ENV = {"HOROVOD_ONESHOT_ALLREDUCE": "1"}

PRELUDE = """
        torch.cuda.set_device(hvd.local_rank() % torch.cuda.device_count())
        dev = torch.device("cuda",
                           hvd.local_rank() % torch.cuda.device_count())
"""

TWO_RANK_BODY = """
        from horovod_amd import _core
        from horovod_amd.torch.sync_batch_norm import native_eligible
        dtype, tol = DTYPE, TOL
        g = torch.Generator().manual_seed(21)
        full = torch.randn(8, 6, 5, 7, generator=g).to(dtype)
        dy_full = torch.randn(8, 6, 5, 7, generator=g).to(dtype)
        wt = torch.rand(6, generator=g) + 0.5
        bs = torch.randn(6, generator=g)
        lo, hi = (0, 3) if rank == 0 else (3, 8)   # uneven batches

        sbn = hvd.SyncBatchNorm(6, momentum=0.3).to(dev)
        with torch.no_grad():
            sbn.weight.copy_(wt)
            sbn.bias.copy_(bs)
        x = full[lo:hi].to(dev).requires_grad_(True)
        assert native_eligible(x)
        out = sbn(x)
        out.backward(dy_full[lo:hi].to(dev))
        torch.cuda.synchronize()

        ref = torch.nn.BatchNorm2d(6, momentum=0.3).double()
        with torch.no_grad():
            ref.weight.copy_(wt)
            ref.bias.copy_(bs)
        xr = full.double().requires_grad_(True)
        yr = ref(xr)
        yr.backward(dy_full.double())

        def close(a, r, t):
            a = a.detach().double().cpu()
            assert torch.allclose(a, r, rtol=t, atol=t), \\
                (a - r).abs().max().item()
        assert out.dtype == dtype
        close(out, yr.detach()[lo:hi], tol)
        close(x.grad, xr.grad[lo:hi], tol)
        close(sbn.running_mean, ref.running_mean, 1e-4)
        close(sbn.running_var, ref.running_var, 1e-3)
        assert not _core.rccl_used(), "stats buffers must stay one-shot"
"""


@requires_gpu
@pytest.mark.parametrize("dtype,tol", [("torch.float32", 2e-4),
                                       ("torch.bfloat16", 5e-2)],
                         ids=["fp32", "bf16"])
def test_two_ranks_uneven_batches(dtype, tol):
    """hvd.SyncBatchNorm over two ranks holding 3 and 5 samples equals
    BatchNorm2d on the concatenated batch."""
    body = TWO_RANK_BODY.replace("DTYPE", dtype).replace("TOL", repr(tol))
    run_workers(2, PRELUDE + body, extra_env=ONESHOT_ENV, timeout=300)
