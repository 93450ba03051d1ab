// Host side of the fused dropout + residual add + LayerNorm kernels
// (ln_kernels.hip), declared in gpu.h.  Every entry point validates all of
// its tensors before the first launch and never falls back to ATen: input the
// kernels do not take raises.  All work goes on torch's current stream with
// no host synchronisation, and the only allocations are the outputs and the
// partial rows of the backward, from torch's allocator.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void LnFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: fused_ln " + what);
}

int LnDType(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DT_F32;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    default: LnFail("supports fp32, fp16 and bf16 activations only");
  }
}

bool Aligned16(const at::Tensor& t) {
  return ((uintptr_t)t.data_ptr() % 16) == 0;
}

// H of an activation the kernels take: a contiguous, 16-B aligned GPU tensor
// whose last dimension is a supported row length.
int64_t CheckActivation(const at::Tensor& x, const char* name) {
  const std::string n(name);
  if (!x.defined()) LnFail("needs " + n);
  if (!x.is_cuda()) LnFail("needs GPU tensors (" + n + " is not one)");
  if (x.dim() < 1 || !x.is_contiguous())
    LnFail("needs a contiguous " + n + " of at least one dimension");
  const int64_t H = x.size(-1);
  if (H < 8 || H > kLnMaxH || H % 8 != 0)
    LnFail("needs a row length H with H % 8 == 0 and 8 <= H <= " +
           std::to_string(kLnMaxH) + ", got " + std::to_string(H));
  if (x.numel() == 0) LnFail("needs at least one row");
  if (!Aligned16(x)) LnFail("needs 16-byte aligned data (" + n + ")");
  return H;
}

// an activation of x's shape, dtype and device
void CheckLike(const at::Tensor& t, const at::Tensor& x, const char* name) {
  CheckActivation(t, name);
  if (t.get_device() != x.get_device() ||
      t.scalar_type() != x.scalar_type() || t.sizes() != x.sizes())
    LnFail(std::string("needs ") + name +
           " of the input's shape, dtype and device");
}

// weight / bias: undefined, or [H] fp32 or of the activations' dtype
void CheckParam(const at::Tensor& w, const at::Tensor& x, int64_t H,
                const char* name) {
  if (!w.defined()) return;
  const std::string n(name);
  if (!w.is_cuda() || w.get_device() != x.get_device())
    LnFail("needs GPU tensors on one device (" + n + ")");
  if (w.scalar_type() != at::kFloat && w.scalar_type() != x.scalar_type())
    LnFail("needs a " + n + " that is fp32 or of the input's dtype");
  if (w.numel() != H || !w.is_contiguous())
    LnFail("needs a contiguous " + n + " of H elements");
  if (!Aligned16(w)) LnFail("needs 16-byte aligned data (" + n + ")");
}

// [M] fp32 row statistics on x's device
void CheckStat(const at::Tensor& s, const at::Tensor& x, int64_t M,
               const char* name) {
  if (!s.defined() || !s.is_cuda() || s.get_device() != x.get_device() ||
      s.scalar_type() != at::kFloat || s.numel() != M || !s.is_contiguous())
    LnFail(std::string("needs ") + name +
           " as a contiguous fp32 GPU tensor with one element per row");
}

LnDropout CheckDropout(double p, uint64_t seed, uint64_t offset) {
  if (!(p >= 0.0 && p <= 1.0)) LnFail("needs 0 <= p <= 1");
  return LnMakeDropout(p, seed, offset);
}

const void* PtrOrNull(const at::Tensor& t) {
  return t.defined() ? t.data_ptr() : nullptr;
}

}  // namespace

std::vector<at::Tensor> FusedLnForward(at::Tensor x, at::Tensor residual,
                                       at::Tensor weight, at::Tensor bias,
                                       double p, double eps, uint64_t seed,
                                       uint64_t offset, bool save_z) {
  const int64_t H = CheckActivation(x, "x");
  const int dt = LnDType(x);
  if (residual.defined()) CheckLike(residual, x, "residual");
  CheckParam(weight, x, H, "weight");
  CheckParam(bias, x, H, "bias");
  const LnDropout d = CheckDropout(p, seed, offset);
  const int64_t M = x.numel() / H;

  const int device = (int)x.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor y = at::empty_like(x);
  // z is x itself without a residual and without dropout
  at::Tensor z;
  if (save_z && (residual.defined() || d.t16 > 0)) z = at::empty_like(x);
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(x.device());
  at::Tensor mean = at::empty({M}, fopts);
  at::Tensor rstd = at::empty({M}, fopts);
  HIP_CHECK(LnForwardLaunch(
      x.data_ptr(), PtrOrNull(residual), PtrOrNull(weight),
      weight.defined() && weight.scalar_type() == at::kFloat, PtrOrNull(bias),
      bias.defined() && bias.scalar_type() == at::kFloat, y.data_ptr(),
      z.defined() ? z.data_ptr() : nullptr, mean.data_ptr<float>(),
      rstd.data_ptr<float>(), M, (int)H, dt, (float)eps, d, stream));
  return {y, z, mean, rstd};
}

std::vector<at::Tensor> FusedLnBackward(at::Tensor dy, at::Tensor z,
                                        at::Tensor mean, at::Tensor rstd,
                                        at::Tensor weight, double p,
                                        uint64_t seed, uint64_t offset,
                                        bool need_wgrad) {
  const int64_t H = CheckActivation(z, "z");
  const int dt = LnDType(z);
  CheckLike(dy, z, "dy");
  CheckParam(weight, z, H, "weight");
  const int64_t M = z.numel() / H;
  CheckStat(mean, z, M, "mean");
  CheckStat(rstd, z, M, "rstd");
  const LnDropout d = CheckDropout(p, seed, offset);

  const int device = (int)z.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor dz = at::empty_like(z);
  // without dropout dx is dz: one tensor for both, written once
  at::Tensor dx = d.t16 > 0 ? at::empty_like(z) : dz;
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(z.device());
  at::Tensor partials, sums;
  int blocks = 0;
  if (need_wgrad) {
    blocks = LnBackwardBlocks(M, (int)H);
    partials = at::empty({blocks, 2 * H}, fopts);
    sums = at::empty({2 * H}, fopts);
  }
  HIP_CHECK(LnBackwardLaunch(
      dy.data_ptr(), z.data_ptr(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), PtrOrNull(weight),
      weight.defined() && weight.scalar_type() == at::kFloat, dz.data_ptr(),
      d.t16 > 0 ? dx.data_ptr() : nullptr,
      need_wgrad ? partials.data_ptr<float>() : nullptr, M, (int)H, dt, d,
      stream));
  at::Tensor dgamma, dbeta;
  if (need_wgrad) {
    HIP_CHECK(LnFoldLaunch(partials.data_ptr<float>(), blocks, (int)H,
                           sums.data_ptr<float>(), stream));
    dgamma = sums.narrow(0, 0, H);
    dbeta = sums.narrow(0, H, H);
  }
  return {dz, dx, dgamma, dbeta};
}

at::Tensor FusedLnKeepMask(int64_t rows, int64_t H, double p, uint64_t seed,
                           uint64_t offset, c10::Device device) {
  if (rows < 1 || H < 8 || H % 8 != 0 || H > (int64_t)1 << 30)
    LnFail("keep mask needs rows >= 1 and H % 8 == 0, H >= 8");
  const LnDropout d = CheckDropout(p, seed, offset);
  auto opts = at::TensorOptions().dtype(at::kByte).device(device);
  if (device.is_cpu()) {
    at::Tensor out = at::empty({rows, H}, opts);
    unsigned char* o = out.data_ptr<unsigned char>();
    const int64_t nvec = rows * (H / 8);
    for (int64_t v = 0; v < nvec; ++v) {
      const unsigned int keep = ln_keep8(d, (unsigned long long)v);
      for (int k = 0; k < 8; ++k) o[v * 8 + k] = (keep >> k) & 1u;
    }
    return out;
  }
  if (!device.is_cuda()) LnFail("keep mask needs a CPU or a GPU device");
  c10::hip::OptionalHIPGuard guard;
  if (device.has_index()) guard.set_index(device.index());
  at::Tensor out = at::empty({rows, H}, opts);
  hipStream_t stream =
      c10::hip::getCurrentHIPStream((int)out.get_device()).stream();
  HIP_CHECK(LnKeepMaskLaunch(out.data_ptr<unsigned char>(), rows, (int)H, d,
                             stream));
  return out;
}

}  // namespace gpu
}  // namespace hvd
