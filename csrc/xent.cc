// Host side of the fused softmax cross-entropy kernels (xent_kernels.hip),
// declared in gpu.h.  As in gelu.cc: every tensor is validated before the
// first launch, input the kernels do not take raises (no ATen fallback), all
// work goes on torch's current stream with no host synchronisation, and the
// only allocations are the outputs.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void XentFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: fused_xent " + what);
}

struct XentShape {
  int64_t M, V;
  int dt, reduction;
};

int Reduction(const std::string& r) {
  if (r == "none") return 0;
  if (r == "mean") return 1;
  if (r == "sum") return 2;
  XentFail("needs reduction 'none', 'mean' or 'sum', got '" + r + "'");
}

XentShape CheckInputs(const at::Tensor& logits, const at::Tensor& labels,
                      double smoothing, const std::string& reduction) {
  if (!logits.defined() || !labels.defined())
    XentFail("needs logits and labels");
  if (!logits.is_cuda() || !labels.is_cuda())
    XentFail("needs GPU tensors (logits and labels)");
  if (labels.get_device() != logits.get_device())
    XentFail("needs logits and labels on one device");
  XentShape s;
  switch (logits.scalar_type()) {
    case at::kFloat: s.dt = DT_F32; break;
    case at::kHalf: s.dt = DT_F16; break;
    case at::kBFloat16: s.dt = DT_BF16; break;
    default: XentFail("supports fp32, fp16 and bf16 logits only");
  }
  if (labels.scalar_type() != at::kLong) XentFail("needs int64 labels");
  if (logits.dim() != 2 || !logits.is_contiguous())
    XentFail("needs contiguous logits of two dimensions, [M, V]");
  s.M = logits.size(0);
  s.V = logits.size(1);
  if (s.M < 1 || s.V < 1) XentFail("needs at least one row and one class");
  if (s.V > kXentMaxV || s.M > kXentMaxM)
    XentFail("takes at most 2^30 classes and 2^31 - 1 rows");
  if (labels.dim() != 1 || labels.size(0) != s.M || !labels.is_contiguous())
    XentFail("needs contiguous labels of M elements");
  if (((uintptr_t)logits.data_ptr() % 16) != 0)
    XentFail("needs 16-byte aligned data (logits)");
  if (!(smoothing >= 0.0 && smoothing < 1.0))
    XentFail("needs 0 <= smoothing < 1");
  s.reduction = Reduction(reduction);
  return s;
}

// fp32, contiguous, n elements, on x's device
void CheckF32(const at::Tensor& t, const at::Tensor& x, int64_t n,
              const char* name) {
  if (!t.defined() || !t.is_cuda() || t.get_device() != x.get_device() ||
      t.scalar_type() != at::kFloat || t.numel() != n || !t.is_contiguous())
    XentFail(std::string("needs ") + name + " as " + std::to_string(n) +
             " contiguous fp32 element(s) on the logits' GPU");
}

}  // namespace

std::vector<at::Tensor> FusedXentForward(at::Tensor logits, at::Tensor labels,
                                         double smoothing,
                                         int64_t ignore_index,
                                         const std::string& reduction) {
  const XentShape s = CheckInputs(logits, labels, smoothing, reduction);
  const int device = (int)logits.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(logits.device());
  at::Tensor lse = at::empty({s.M}, fopts);
  at::Tensor row_loss = at::empty({s.M}, fopts);
  at::Tensor folded = at::empty({2}, fopts);  // {loss, count}
  const long long* y = (const long long*)labels.data_ptr();
  HIP_CHECK(XentForwardLaunch(logits.data_ptr(), y, lse.data_ptr<float>(),
                              row_loss.data_ptr<float>(), s.M, (int)s.V, s.dt,
                              (float)smoothing, ignore_index, stream));
  HIP_CHECK(XentFoldLaunch(row_loss.data_ptr<float>(), y, s.M, ignore_index,
                           s.reduction == 1, folded.data_ptr<float>(),
                           stream));
  at::Tensor count = folded.select(0, 1);
  if (s.reduction == 0) return {row_loss, at::Tensor(), lse, count};
  return {folded.select(0, 0), row_loss, lse, count};
}

at::Tensor FusedXentBackward(at::Tensor dloss, at::Tensor logits,
                             at::Tensor labels, at::Tensor lse,
                             at::Tensor count, double smoothing,
                             int64_t ignore_index,
                             const std::string& reduction) {
  const XentShape s = CheckInputs(logits, labels, smoothing, reduction);
  CheckF32(dloss, logits, s.reduction == 0 ? s.M : 1, "dloss");
  CheckF32(lse, logits, s.M, "lse");
  CheckF32(count, logits, 1, "count");
  const int device = (int)logits.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor dx = at::empty_like(logits);
  if (((uintptr_t)dx.data_ptr() % 16) != 0)
    XentFail("needs 16-byte aligned data (dx)");
  HIP_CHECK(XentBackwardLaunch(
      logits.data_ptr(), (const long long*)labels.data_ptr(),
      lse.data_ptr<float>(), dloss.data_ptr<float>(),
      count.data_ptr<float>(), dx.data_ptr(), s.M, (int)s.V, s.dt,
      (float)smoothing, ignore_index, s.reduction, stream));
  return dx;
}

int64_t FusedXentWaveMaxV() { return kXentWaveMaxV; }

// ---- with the bias folded in (xent_bias_kernels.hip) ------------------------
// Next to the outputs the forward allocates the shifted copies of the bias its
// kernel reads, and the backward the partial rows of the bias gradient.

namespace {

void CheckBias(const at::Tensor& bias, const at::Tensor& logits, int64_t V) {
  if (!bias.defined() || !bias.is_cuda() ||
      bias.get_device() != logits.get_device() ||
      bias.scalar_type() != at::kFloat || bias.dim() != 1 ||
      bias.size(0) != V || !bias.is_contiguous())
    XentFail("needs bias as " + std::to_string(V) +
             " contiguous fp32 elements, [V], on the logits' GPU");
}

}  // namespace

std::vector<at::Tensor> FusedXentBiasForward(at::Tensor logits,
                                             at::Tensor bias,
                                             at::Tensor labels,
                                             double smoothing,
                                             int64_t ignore_index,
                                             const std::string& reduction) {
  const XentShape s = CheckInputs(logits, labels, smoothing, reduction);
  CheckBias(bias, logits, s.V);
  const int device = (int)logits.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(logits.device());
  at::Tensor lse = at::empty({s.M}, fopts);
  at::Tensor row_loss = at::empty({s.M}, fopts);
  at::Tensor folded = at::empty({2}, fopts);  // {loss, count}
  at::Tensor shift = at::empty(
      {XentBiasPhases((int)s.V, s.dt), XentBiasPitch((int)s.V)}, fopts);
  if (((uintptr_t)shift.data_ptr() % 16) != 0)
    XentFail("needs 16-byte aligned data (shifted bias)");
  const long long* y = (const long long*)labels.data_ptr();
  HIP_CHECK(XentBiasForwardLaunch(
      logits.data_ptr(), bias.data_ptr<float>(), y, shift.data_ptr<float>(),
      lse.data_ptr<float>(), row_loss.data_ptr<float>(), s.M, (int)s.V, s.dt,
      (float)smoothing, ignore_index, stream));
  HIP_CHECK(XentFoldLaunch(row_loss.data_ptr<float>(), y, s.M, ignore_index,
                           s.reduction == 1, folded.data_ptr<float>(),
                           stream));
  at::Tensor count = folded.select(0, 1);
  if (s.reduction == 0) return {row_loss, at::Tensor(), lse, count};
  return {folded.select(0, 0), row_loss, lse, count};
}

std::vector<at::Tensor> FusedXentBiasBackward(at::Tensor dloss,
                                              at::Tensor logits,
                                              at::Tensor bias,
                                              at::Tensor labels,
                                              at::Tensor lse, at::Tensor count,
                                              double smoothing,
                                              int64_t ignore_index,
                                              const std::string& reduction) {
  const XentShape s = CheckInputs(logits, labels, smoothing, reduction);
  CheckBias(bias, logits, s.V);
  CheckF32(dloss, logits, s.reduction == 0 ? s.M : 1, "dloss");
  CheckF32(lse, logits, s.M, "lse");
  CheckF32(count, logits, 1, "count");
  const int device = (int)logits.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor dx = at::empty_like(logits);
  if (((uintptr_t)dx.data_ptr() % 16) != 0)
    XentFail("needs 16-byte aligned data (dx)");
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(logits.device());
  const int64_t rows = (int64_t)XentBiasPhases((int)s.V, s.dt) *
                       XentBiasRowChunks(s.M, (int)s.V, s.dt);
  at::Tensor dbias = at::empty({s.V}, fopts);
  // a single partial row is the gradient itself
  at::Tensor partials = rows == 1 ? dbias : at::empty({rows, s.V}, fopts);
  HIP_CHECK(XentBiasBackwardLaunch(
      logits.data_ptr(), bias.data_ptr<float>(),
      (const long long*)labels.data_ptr(), lse.data_ptr<float>(),
      dloss.data_ptr<float>(), count.data_ptr<float>(), dx.data_ptr(),
      partials.data_ptr<float>(), s.M, (int)s.V, s.dt, (float)smoothing,
      ignore_index, s.reduction, stream));
  if (rows > 1)
    HIP_CHECK(ColumnFoldLaunch(partials.data_ptr<float>(), (int)rows, (int)s.V,
                               dbias.data_ptr<float>(), stream));
  return {dx, dbias};
}

int64_t FusedXentBiasRowChunks(int64_t M, int64_t V, at::ScalarType dtype) {
  if (M < 1 || V < 1 || V > kXentMaxV || M > kXentMaxM)
    XentFail("row chunks need 1 <= M <= 2^31 - 1 and 1 <= V <= 2^30");
  int dt;
  switch (dtype) {
    case at::kFloat: dt = DT_F32; break;
    case at::kHalf: dt = DT_F16; break;
    case at::kBFloat16: dt = DT_BF16; break;
    default: XentFail("supports fp32, fp16 and bf16 logits only");
  }
  return XentBiasRowChunks(M, (int)V, dt);
}

}  // namespace gpu
}  // namespace hvd
