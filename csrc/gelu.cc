// Host side of the fused bias + GELU + dropout kernels (gelu_kernels.hip),
// declared in gpu.h.  As in ln.cc: every tensor is validated before the first
// launch, input the kernels do not take raises (no ATen fallback), all work
// goes on torch's current stream with no host synchronisation, and the only
// allocations are the outputs and the partial rows of the bias gradient.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void GeluFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: fused_bias_gelu " + what);
}

bool Aligned16(const at::Tensor& t) {
  return ((uintptr_t)t.data_ptr() % 16) == 0;
}

// N of an activation the kernels take: a contiguous, 16-B aligned fp32 / fp16
// / bf16 GPU tensor whose last dimension is a multiple of 8.
int64_t CheckActivation(const at::Tensor& x, const char* name) {
  const std::string n(name);
  if (!x.defined()) GeluFail("needs " + n);
  if (!x.is_cuda()) GeluFail("needs GPU tensors (" + n + " is not one)");
  if (x.scalar_type() != at::kFloat && x.scalar_type() != at::kHalf &&
      x.scalar_type() != at::kBFloat16)
    GeluFail("supports fp32, fp16 and bf16 activations only");
  if (x.dim() < 1 || !x.is_contiguous())
    GeluFail("needs a contiguous " + n + " of at least one dimension");
  const int64_t N = x.size(-1);
  if (N < 8 || N > kGeluMaxN || N % 8 != 0)
    GeluFail("needs a row length N with N % 8 == 0 and N >= 8, got " +
             std::to_string(N));
  if (x.numel() == 0) GeluFail("needs at least one row");
  if (!Aligned16(x)) GeluFail("needs 16-byte aligned data (" + n + ")");
  return N;
}

// bias: undefined, or [N] fp32 or of the activations' dtype
void CheckBias(const at::Tensor& b, const at::Tensor& x, int64_t N) {
  if (!b.defined()) return;
  if (!b.is_cuda() || b.get_device() != x.get_device())
    GeluFail("needs GPU tensors on one device (bias)");
  if (b.scalar_type() != at::kFloat && b.scalar_type() != x.scalar_type())
    GeluFail("needs a bias that is fp32 or of the input's dtype");
  if (b.numel() != N || !b.is_contiguous())
    GeluFail("needs a contiguous bias of N elements");
  if (!Aligned16(b)) GeluFail("needs 16-byte aligned data (bias)");
}

LnDropout CheckDropout(double p, uint64_t seed, uint64_t offset) {
  if (!(p >= 0.0 && p <= 1.0)) GeluFail("needs 0 <= p <= 1");
  return LnMakeDropout(p, seed, offset);
}

int DType(const at::Tensor& t) {
  return t.scalar_type() == at::kFloat
             ? DT_F32
             : (t.scalar_type() == at::kHalf ? DT_F16 : DT_BF16);
}

const void* PtrOrNull(const at::Tensor& t) {
  return t.defined() ? t.data_ptr() : nullptr;
}

bool IsF32(const at::Tensor& t) {
  return t.defined() && t.scalar_type() == at::kFloat;
}

}  // namespace

at::Tensor FusedBiasGeluForward(at::Tensor u, at::Tensor bias, double p,
                                uint64_t seed, uint64_t offset, bool tanh) {
  const int64_t N = CheckActivation(u, "u");
  CheckBias(bias, u, N);
  const LnDropout d = CheckDropout(p, seed, offset);
  const int64_t M = u.numel() / N;

  const int device = (int)u.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor out = at::empty_like(u);
  HIP_CHECK(GeluForwardLaunch(u.data_ptr(), PtrOrNull(bias), IsF32(bias),
                              out.data_ptr(), M, (int)N, DType(u), tanh, d,
                              stream));
  return out;
}

std::vector<at::Tensor> FusedBiasGeluBackward(at::Tensor dy, at::Tensor u,
                                              at::Tensor bias, double p,
                                              uint64_t seed, uint64_t offset,
                                              bool tanh,
                                              bool need_bias_grad) {
  const int64_t N = CheckActivation(u, "u");
  CheckActivation(dy, "dy");
  if (dy.get_device() != u.get_device() ||
      dy.scalar_type() != u.scalar_type() || dy.sizes() != u.sizes())
    GeluFail("needs dy of u's shape, dtype and device");
  CheckBias(bias, u, N);
  const LnDropout d = CheckDropout(p, seed, offset);
  const int64_t M = u.numel() / N;

  const int device = (int)u.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor du = at::empty_like(u);
  const int chunks = GeluRowChunks(M, (int)N);
  at::Tensor partials, dbias;
  if (need_bias_grad) {
    auto fopts = at::TensorOptions().dtype(at::kFloat).device(u.device());
    dbias = at::empty({N}, fopts);
    // a single partial row is the gradient itself
    partials = chunks == 1 ? dbias : at::empty({chunks, N}, fopts);
  }
  HIP_CHECK(GeluBackwardLaunch(
      dy.data_ptr(), u.data_ptr(), PtrOrNull(bias), IsF32(bias),
      du.data_ptr(), need_bias_grad ? partials.data_ptr<float>() : nullptr,
      chunks, M, (int)N, DType(u), tanh, d, stream));
  if (need_bias_grad && chunks > 1)
    HIP_CHECK(ColumnFoldLaunch(partials.data_ptr<float>(), chunks, (int)N,
                               dbias.data_ptr<float>(), stream));
  return {du, dbias};
}

int64_t FusedBiasGeluRowChunks(int64_t M, int64_t N) {
  if (M < 1 || N < 8 || N > kGeluMaxN || N % 8 != 0)
    GeluFail("row chunks need M >= 1 and N % 8 == 0, N >= 8");
  return GeluRowChunks(M, (int)N);
}

}  // namespace gpu
}  // namespace hvd
