// Host side of the row compaction kernels (rows_kernels.hip), declared in
// gpu.h.  As in emb.cc: every tensor is validated before the first launch,
// input the kernels do not take raises (no ATen fallback), all work goes on
// torch's current stream with no host synchronisation, and the only
// allocations are the outputs and the per-chunk counts of a long label array.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void RowsFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: masked_rows " + what);
}

// a contiguous GPU tensor of `type` with n elements (any n when n < 0)
void CheckVector(const at::Tensor& t, at::ScalarType type, int64_t n,
                 size_t align, const char* name) {
  if (!t.defined() || !t.is_cuda())
    RowsFail(std::string("needs GPU tensors (") + name + ")");
  if (t.scalar_type() != type || !t.is_contiguous() || t.numel() < 1 ||
      (n >= 0 && t.numel() != n) || t.numel() > kRowsMaxM ||
      ((uintptr_t)t.data_ptr() % align) != 0)
    RowsFail(std::string("needs ") + name + " as a contiguous, " +
             std::to_string(align) + "-byte aligned " + c10::toString(type) +
             " tensor" +
             (n >= 0 ? " of " + std::to_string(n) + " element(s)" : ""));
}

int RowsDType(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return DT_F32;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    default: RowsFail("supports fp32, fp16 and bf16 rows only");
  }
}

// [n, H] rows of 16-B vectors next to `like`; -> bytes of a row
int64_t CheckRows(const at::Tensor& x, const at::Tensor& like,
                  const char* name) {
  const std::string n(name);
  if (!x.defined() || !x.is_cuda())
    RowsFail("needs GPU tensors (" + n + ")");
  if (x.get_device() != like.get_device())
    RowsFail("needs its tensors on one device (" + n + ")");
  RowsDType(x.scalar_type());
  if (x.dim() != 2 || x.size(0) < 1 || x.size(0) > kRowsMaxM ||
      !x.is_contiguous() || ((uintptr_t)x.data_ptr() % 16) != 0)
    RowsFail("needs " + n + " as contiguous, 16-byte aligned rows [n, H]");
  const int64_t bytes = x.size(1) * (int64_t)x.element_size();
  if (bytes < 16 || bytes % 16 != 0 || bytes > kRowsMaxRowBytes)
    RowsFail("needs rows of a multiple of 16 bytes, at most " +
             std::to_string(kRowsMaxRowBytes) + ", got " +
             std::to_string(bytes));
  return bytes;
}

}  // namespace

std::vector<at::Tensor> MaskedRowsIndex(at::Tensor labels, int64_t capacity,
                                        int64_t ignore_index,
                                        int64_t launches) {
  CheckVector(labels, at::kLong, -1, 16, "labels");
  if (capacity < 1 || capacity > kRowsMaxM)
    RowsFail("needs 1 <= capacity < 2^31");
  if (launches < 0 || launches > 2) RowsFail("needs launches 0, 1 or 2");
  const int64_t M = labels.numel();

  const int device = (int)labels.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto iopts = at::TensorOptions().dtype(at::kInt).device(labels.device());
  at::Tensor idx = at::empty({capacity}, iopts);
  at::Tensor rank = at::empty({M}, iopts);
  at::Tensor row_labels = at::empty({capacity}, labels.options());
  at::Tensor count = at::empty({1}, iopts);
  at::Tensor counts;
  if (launches == 2 || (launches == 0 && RowsIndexUsesCounts(M)))
    counts = at::empty({RowsIndexChunks(M)}, iopts);
  HIP_CHECK(RowsIndexLaunch(
      (const long long*)labels.data_ptr<int64_t>(), M, ignore_index, capacity,
      counts.defined() ? counts.data_ptr<int>() : nullptr,
      idx.data_ptr<int>(), rank.data_ptr<int>(),
      (long long*)row_labels.data_ptr<int64_t>(), count.data_ptr<int>(),
      stream));
  return {idx, rank, row_labels, count};
}

at::Tensor MaskedRowsGather(at::Tensor x, at::Tensor idx, at::Tensor count) {
  CheckVector(idx, at::kInt, -1, 4, "idx");
  const int64_t bytes = CheckRows(x, idx, "x");
  CheckVector(count, at::kInt, 1, 4, "count");
  if (count.get_device() != idx.get_device())
    RowsFail("needs its tensors on one device (count)");
  const int64_t capacity = idx.numel();

  const int device = (int)x.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor rows = at::empty({capacity, x.size(1)}, x.options());
  HIP_CHECK(RowsGatherLaunch(x.data_ptr(), idx.data_ptr<int>(),
                             count.data_ptr<int>(), rows.data_ptr(),
                             x.size(0), capacity, bytes,
                             RowsDType(x.scalar_type()), stream));
  return rows;
}

at::Tensor MaskedRowsScatter(at::Tensor d_rows, at::Tensor rank) {
  CheckVector(rank, at::kInt, -1, 4, "rank");
  const int64_t bytes = CheckRows(d_rows, rank, "d_rows");
  const int64_t M = rank.numel();

  const int device = (int)d_rows.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor dx = at::empty({M, d_rows.size(1)}, d_rows.options());
  HIP_CHECK(RowsScatterLaunch(d_rows.data_ptr(), rank.data_ptr<int>(),
                              dx.data_ptr(), M, d_rows.size(0), bytes,
                              stream));
  return dx;
}

int64_t MaskedRowsChunk() { return kRowsChunk; }

}  // namespace gpu
}  // namespace hvd
