"""The native SyncBatchNorm surface exists after build() and the path
selector keeps CPU / fp64 tensors on the composite code (no GPU needed)."""
import torch


def test_core_exports_sync_bn_symbols():
    from horovod_amd import _core
    for name in ("sync_bn_stats", "sync_bn_normalize",
                 "sync_bn_backward_reduce", "sync_bn_backward_apply"):
        assert callable(getattr(_core, name, None)), name


def test_native_eligible_false_on_cpu_and_fp64():
    from horovod_amd.torch.sync_batch_norm import native_eligible
    assert native_eligible(torch.randn(4, 3, 5, 5)) is False
    assert native_eligible(torch.randn(4, 3, 5, 5,
                                       dtype=torch.bfloat16)) is False
    assert native_eligible(torch.randn(4, 3, 5, 5,
                                       dtype=torch.float64)) is False
    if torch.cuda.is_available():
        x = torch.randn(4, 3, 5, 5, dtype=torch.float64, device="cuda")
        assert native_eligible(x) is False
