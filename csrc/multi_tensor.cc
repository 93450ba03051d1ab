// Host side of the multi-tensor kernels: global-norm clipping
// (clip_kernels.hip) and the fused SGD / AdamW / LAMB / LARS steps
// (sgd_kernels.hip, adamw_kernels.hip, lamb_kernels.hip, lars_kernels.hip),
// declared in gpu.h.
// Every entry point validates all of its tensors before the first launch (a
// throw must not leave half of them updated), then fills descriptor batches
// (MultiTensorArgs, kernels.h) through a Batcher, on torch's current stream.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <functional>
#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

using TensorList = std::vector<at::Tensor>;
// Parallel lists: tensor i of list r goes to pointer row r of a descriptor.
using Rows = std::vector<const TensorList*>;

// Device pointer of an optional 1-element device tensor of type T (a clip
// coefficient, a skip flag, a loss scale, ...): undefined -> null.
template <typename T = float>
T* ScalarPtr(const at::Tensor& t, int device, const char* name,
             const char* where = "parameters'") {
  if (!t.defined()) return nullptr;
  if (!t.is_cuda() || t.get_device() != device ||
      t.scalar_type() != c10::CppTypeToScalarType<T>::value || t.numel() != 1)
    throw std::runtime_error(
        std::string("horovod_amd: ") + name + " must be a 1-element " +
        (std::is_same<T, float>::value ? "fp32" : "int32") +
        " tensor on the " + where + " device");
  return t.data_ptr<T>();
}

const float* GradCoefPtr(const at::Tensor& coef, int device) {
  return ScalarPtr(coef, device, "grad_coef");
}
const float* SkipPtr(const at::Tensor& skip, int device) {
  return ScalarPtr(skip, device, "skip");
}

struct TupleInfo {
  int device;            // of every tensor (the current one without tensors)
  int64_t chunk_blocks;  // sum of ChunkBlocks over the tuples
  bool any_empty;
};

// What the optimizer kernels need of the tuples (rows[0][i], rows[1][i], ...),
// rows[0] being the parameters, rows[1] the gradients and `others` naming the
// rest: lists of one length, dense fp32 tensors on one GPU, each tuple of one
// size and layout (the kernels walk memory order), and for `chunked` kernels
// the size limit.  With `models` (master weights) rows[0] are the fp32
// masters, and models[i] and its gradient share one 2-byte dtype.
TupleInfo CheckTuples(const std::string& op, const char* others,
                      const Rows& rows, bool chunked,
                      const TensorList* models = nullptr) {
  auto fail = [&op](const std::string& what) {
    throw std::runtime_error("horovod_amd: " + op + what);
  };
  const TensorList& params = *rows[0];
  const size_t n = params.size();
  for (const TensorList* list : rows)
    if (list->size() != n)
      fail(std::string(" needs as many ") + others + " as params");
  if (models && models->size() != n)
    fail(" needs as many model_params as params");
  Rows all = rows;
  if (models) all.push_back(models);
  TupleInfo info{n == 0 ? (int)c10::hip::current_device() : -1, 0, false};
  for (size_t i = 0; i < n; ++i) {
    const at::Tensor& p = params[i];
    if (models && (*models)[i].scalar_type() != at::kHalf &&
        (*models)[i].scalar_type() != at::kBFloat16)
      fail(" needs fp16 or bf16 model_params");
    for (const TensorList* list : all) {
      const at::Tensor& t = (*list)[i];
      if (info.device < 0 && t.is_cuda()) info.device = (int)t.get_device();
      if (!t.is_cuda() || t.is_sparse() || t.get_device() != info.device)
        fail(" needs dense tensors on one GPU");
      if (!models) {
        if (t.scalar_type() != at::kFloat) fail(" supports fp32 tensors only");
      } else if (list == rows[1]) {
        if (t.scalar_type() != (*models)[i].scalar_type())
          fail(" needs a gradient of its model parameter's dtype");
      } else if (list != models && t.scalar_type() != at::kFloat) {
        fail(" with model_params needs fp32 masters and moments");
      }
      const bool same_layout =
          (t.is_contiguous() && p.is_contiguous()) ||
          (t.sizes() == p.sizes() && t.strides() == p.strides());
      if (!t.is_non_overlapping_and_dense() || t.numel() != p.numel() ||
          !same_layout)
        fail(" needs a parameter, its gradient and its moments to be dense "
             "tensors of one size and layout");
    }
    // one tensor too large for a launch's 32-bit block index
    if (chunked && p.numel() / kChunkElems >= (int64_t)1 << 30)
      fail(": tensor too large");
    info.chunk_blocks += ChunkBlocks(p.numel());
    info.any_empty = info.any_empty || p.numel() == 0;
  }
  return info;
}

// Fills descriptors one tensor tuple at a time and hands every batch to
// `launch`: when it is full, when a chunked one would pass 2^30 blocks, and
// at the final Flush().  Empty tensors take no descriptor.
template <typename Args>
class Batcher {
 public:
  explicit Batcher(std::function<void(Args&)> launch)
      : launch_(std::move(launch)) {}

  // Tuple i of `rows` (a null row gives null pointers); `index`: its slot in
  // an indexed per-tensor output.
  void Add(const Rows& rows, size_t i, unsigned int index = 0) {
    const int64_t numel = (*rows[0])[i].numel();
    if (numel == 0) return;
    if (args_.count == kCopyBatchCapacity) Flush();
    const int64_t blocks = ChunkBlocks(numel);
    if constexpr (Args::kChunked) {
      if ((int64_t)args_.block_prefix[args_.count] + blocks > (int64_t)1 << 30)
        Flush();
    }
    const int k = args_.count++;
    for (size_t r = 0; r < (size_t)Args::kRows; ++r)
      args_.ptr[r][k] =
          r < rows.size() && rows[r] ? (*rows[r])[i].data_ptr() : nullptr;
    args_.numel[k] = (unsigned long long)numel;
    if constexpr (Args::kChunked)
      args_.block_prefix[k + 1] = args_.block_prefix[k] + (unsigned int)blocks;
    if constexpr (Args::kIndexed) args_.out_index[k] = index;
  }

  void Flush() {
    if (args_.count == 0) return;
    launch_(args_);
    args_.count = 0;
  }

 private:
  Args args_;
  std::function<void(Args&)> launch_;
};

int ClipDevice(const at::Tensor& first) {
  if (!first.is_cuda())
    throw std::runtime_error(
        "horovod_amd: clip kernels need dense tensors on one GPU");
  return (int)first.get_device();
}

// Dense fp32/fp16/bf16 tensors of one device -> launches of one dtype each.
// launch(args, dt) gets block_prefix filled in.
void ForEachClipBatch(const TensorList& tensors, int device,
                      const std::function<void(ClipBatchArgs&, int)>& launch) {
  for (const auto& t : tensors) {
    if (!t.is_cuda() || t.get_device() != device || t.is_sparse() ||
        !t.is_non_overlapping_and_dense())
      throw std::runtime_error(
          "horovod_amd: clip kernels need dense tensors on one GPU");
    if (t.scalar_type() != at::kFloat && t.scalar_type() != at::kHalf &&
        t.scalar_type() != at::kBFloat16)
      throw std::runtime_error(
          "horovod_amd: clip kernels support fp32, fp16 and bf16");
    // one tensor too large for a launch's 32-bit block index
    if (t.numel() / kChunkElems >= (int64_t)1 << 30)
      throw std::runtime_error("horovod_amd: tensor too large to clip");
  }
  auto of = [&launch](int dt) {
    return Batcher<ClipBatchArgs>(
        [&launch, dt](ClipBatchArgs& args) { launch(args, dt); });
  };
  Batcher<ClipBatchArgs> batch[3] = {of(DT_F32), of(DT_F16), of(DT_BF16)};
  const Rows rows{&tensors};
  for (size_t i = 0; i < tensors.size(); ++i) {
    const auto dt = tensors[i].scalar_type();
    batch[dt == at::kFloat ? 0 : dt == at::kHalf ? 1 : 2].Add(rows, i);
  }
  for (auto& b : batch) b.Flush();
}

// Master weights: one launch handles one 2-byte dtype, so the tuples go to a
// Batcher per dtype.  launch(args, dt) as above; rows.back() are the model
// parameters.
template <typename Args>
void ForEachMasterBatch(const Rows& rows, bool indexed,
                        const std::function<void(Args&, int)>& launch) {
  auto of = [&launch](int dt) {
    return Batcher<Args>([&launch, dt](Args& args) { launch(args, dt); });
  };
  Batcher<Args> batch[2] = {of(DT_F16), of(DT_BF16)};
  const TensorList& models = *rows.back();
  for (size_t i = 0; i < models.size(); ++i)
    batch[models[i].scalar_type() == at::kHalf ? 0 : 1].Add(
        rows, i, indexed ? (unsigned int)i : 0);
  for (auto& b : batch) b.Flush();
}

}  // namespace

at::Tensor MultiTensorGradNorm(std::vector<at::Tensor>& grads,
                               double max_norm) {
  int device = grads.empty() ? (int)c10::hip::current_device()
                             : ClipDevice(grads[0]);
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device);
  int64_t total_blocks = 0;
  for (const auto& g : grads) total_blocks += ChunkBlocks(g.numel());
  // every slot is written by exactly one block before the finalize reads it
  at::Tensor partials = at::empty({std::max<int64_t>(total_blocks, 1)}, f32);
  at::Tensor out = at::empty({2}, f32);
  unsigned long long base = 0;
  ForEachClipBatch(grads, device, [&](ClipBatchArgs& args, int dt) {
    args.partial_base = base;
    HIP_CHECK(MultiSqNormLaunch(args, dt, partials.data_ptr<float>(), stream));
    base += args.block_prefix[args.count];
  });
  HIP_CHECK(ClipFinalizeLaunch(partials.data_ptr<float>(), (long long)base,
                               (float)max_norm, out.data_ptr<float>(),
                               stream));
  return out;
}

at::Tensor MultiTensorScaledGradNorm(std::vector<at::Tensor>& grads,
                                     std::optional<double> max_norm,
                                     at::Tensor scale, at::Tensor found_inf,
                                     at::Tensor growth_tracker,
                                     double growth_factor,
                                     double backoff_factor,
                                     int64_t growth_interval) {
  // without gradients: the device of whichever tensor is given
  int device = !grads.empty()        ? ClipDevice(grads[0])
               : scale.defined()     ? ClipDevice(scale)
               : found_inf.defined() ? ClipDevice(found_inf)
                                     : (int)c10::hip::current_device();
  ScaledFinalizeParams p;
  p.has_max_norm = max_norm.has_value();
  p.max_norm = (float)max_norm.value_or(0.0);
  p.scale = ScalarPtr(scale, device, "scale", "gradients'");
  p.found_inf = ScalarPtr(found_inf, device, "found_inf", "gradients'");
  p.growth_tracker =
      ScalarPtr<int>(growth_tracker, device, "growth_tracker", "gradients'");
  p.growth_factor = (float)growth_factor;
  p.backoff_factor = (float)backoff_factor;
  if (p.growth_tracker && !p.scale)
    throw std::runtime_error(
        "horovod_amd: growth_tracker needs a scale to update");
  if (growth_interval < 0 || growth_interval > INT32_MAX)
    throw std::runtime_error("horovod_amd: growth_interval out of range");
  p.growth_interval = (int)growth_interval;
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device);
  int64_t total_blocks = 0;
  for (const auto& g : grads) total_blocks += ChunkBlocks(g.numel());
  // every slot is written by exactly one block before the finalize reads it
  at::Tensor partials = at::empty({std::max<int64_t>(total_blocks, 1)}, f32);
  at::Tensor out = at::empty({4}, f32);
  unsigned long long base = 0;
  // checks every gradient before its first launch
  ForEachClipBatch(grads, device, [&](ClipBatchArgs& args, int dt) {
    args.partial_base = base;
    HIP_CHECK(MultiSqNormLaunch(args, dt, partials.data_ptr<float>(), stream));
    base += args.block_prefix[args.count];
  });
  HIP_CHECK(ScaledClipFinalizeLaunch(partials.data_ptr<float>(),
                                     (long long)base, p,
                                     out.data_ptr<float>(), stream));
  return out;
}

void MultiTensorScale(std::vector<at::Tensor>& tensors, at::Tensor coef) {
  if (tensors.empty()) return;
  int device = ClipDevice(tensors[0]);
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  const float* c = GradCoefPtr(coef, device);
  if (!c) throw std::runtime_error("horovod_amd: coef must be defined");
  ForEachClipBatch(tensors, device, [&](ClipBatchArgs& args, int dt) {
    HIP_CHECK(MultiScaleLaunch(args, dt, c, stream));
  });
}

void FusedSgdStep(std::vector<at::Tensor>& params,
                  std::vector<at::Tensor>& grads,
                  std::vector<at::Tensor>& momenta, double lr, double momentum,
                  double weight_decay, double dampening, bool nesterov,
                  at::Tensor grad_coef,
                  const std::vector<at::Tensor>* model_params,
                  at::Tensor skip) {
  // the kernel reads the momentum row exactly when the launcher sees a
  // nonzero fp32 momentum; without it `momenta` is not looked at
  const bool use_momentum = (float)momentum != 0.0f;
  Rows rows{&params, &grads};
  if (use_momentum) rows.push_back(&momenta);
  const TupleInfo info = CheckTuples(
      "fused_sgd_step", use_momentum ? "grads and momenta" : "grads", rows,
      false, model_params);
  if (params.empty()) return;
  c10::hip::HIPGuard guard(info.device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(info.device).stream();
  const float* coef = GradCoefPtr(grad_coef, info.device);
  const float* skip_ptr = SkipPtr(skip, info.device);
  if (model_params) {
    rows = {&params, &grads, use_momentum ? &momenta : nullptr, model_params};
    ForEachMasterBatch<SgdMasterBatchArgs>(
        rows, false, [&](SgdMasterBatchArgs& args, int dt) {
          HIP_CHECK(FusedSgdMasterLaunch(args, dt, (float)lr, (float)momentum,
                                         (float)weight_decay,
                                         (float)dampening, nesterov, coef,
                                         skip_ptr, stream));
        });
    return;
  }
  Batcher<SgdBatchArgs> batch([&](SgdBatchArgs& args) {
    HIP_CHECK(FusedSgdLaunch(args, (float)lr, (float)momentum,
                             (float)weight_decay, (float)dampening, nesterov,
                             coef, skip_ptr, stream));
  });
  for (size_t i = 0; i < params.size(); ++i) batch.Add(rows, i);
  batch.Flush();
}

void FusedAdamwStep(std::vector<at::Tensor>& params,
                    std::vector<at::Tensor>& grads,
                    std::vector<at::Tensor>& exp_avgs,
                    std::vector<at::Tensor>& exp_avg_sqs, double lr,
                    double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, at::Tensor grad_coef,
                    const std::vector<at::Tensor>* model_params,
                    at::Tensor skip) {
  Rows rows{&params, &grads, &exp_avgs, &exp_avg_sqs};
  const TupleInfo info =
      CheckTuples("fused_adamw_step", "grads, exp_avgs and exp_avg_sqs", rows,
                  false, model_params);
  if (params.empty()) return;
  c10::hip::HIPGuard guard(info.device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(info.device).stream();
  const float* coef = GradCoefPtr(grad_coef, info.device);
  const float* skip_ptr = SkipPtr(skip, info.device);
  if (model_params) {
    rows.push_back(model_params);
    ForEachMasterBatch<AdamwMasterBatchArgs>(
        rows, false, [&](AdamwMasterBatchArgs& args, int dt) {
          HIP_CHECK(FusedAdamwMasterLaunch(args, dt, (float)lr, (float)beta1,
                                           (float)beta2, (float)eps,
                                           (float)weight_decay, step, coef,
                                           skip_ptr, stream));
        });
    return;
  }
  Batcher<AdamwBatchArgs> batch([&](AdamwBatchArgs& args) {
    HIP_CHECK(FusedAdamwLaunch(args, (float)lr, (float)beta1, (float)beta2,
                               (float)eps, (float)weight_decay, step, coef,
                               skip_ptr, stream));
  });
  for (size_t i = 0; i < params.size(); ++i) batch.Add(rows, i);
  batch.Flush();
}

at::Tensor FusedLambStep(std::vector<at::Tensor>& params,
                         std::vector<at::Tensor>& grads,
                         std::vector<at::Tensor>& exp_avgs,
                         std::vector<at::Tensor>& exp_avg_sqs, double lr,
                         double beta1, double beta2, double eps,
                         double weight_decay, int64_t step,
                         bool bias_correction, bool adapt,
                         at::Tensor grad_coef,
                         const std::vector<at::Tensor>* model_params,
                         at::Tensor skip) {
  Rows rows{&params, &grads, &exp_avgs, &exp_avg_sqs};
  const TupleInfo info =
      CheckTuples("fused_lamb_step", "grads, exp_avgs and exp_avg_sqs", rows,
                  true, model_params);
  if (step < 1)
    throw std::runtime_error("horovod_amd: fused_lamb_step: step is 1-based");
  const int64_t n = (int64_t)params.size();
  c10::hip::HIPGuard guard(info.device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(info.device).stream();
  const float* coef = GradCoefPtr(grad_coef, info.device);
  const float* skip_ptr = SkipPtr(skip, info.device);
  auto f32 =
      at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, info.device);
  // sized for the whole call; every slot is written by exactly one block
  // before the trust kernel of its batch reads it
  at::Tensor partials =
      at::empty({std::max<int64_t>(2 * info.chunk_blocks, 1)}, f32);
  // empty tensors take no descriptor: their ratio is the preset 1
  at::Tensor trust = info.any_empty ? at::ones({n}, f32) : at::empty({n}, f32);
  const LambScalars s =
      LambFoldScalars((float)lr, (float)beta1, (float)beta2, (float)eps,
                      (float)weight_decay, step, bias_correction);
  unsigned long long base = 0;
  if (model_params) {
    rows.push_back(model_params);
    ForEachMasterBatch<LambMasterBatchArgs>(
        rows, true, [&](LambMasterBatchArgs& args, int dt) {
          args.partial_base = base;
          HIP_CHECK(LambMomentsMasterLaunch(args, dt, s, coef, skip_ptr,
                                            partials.data_ptr<float>(),
                                            stream));
          HIP_CHECK(LambTrustLaunch(args, partials.data_ptr<float>(), adapt,
                                    skip_ptr, trust.data_ptr<float>(),
                                    stream));
          HIP_CHECK(LambUpdateMasterLaunch(
              args, dt, s, trust.data_ptr<float>(), skip_ptr, stream));
          base += args.block_prefix[args.count];
        });
    return trust;
  }
  Batcher<LambBatchArgs> batch([&](LambBatchArgs& args) {
    args.partial_base = base;
    HIP_CHECK(LambMomentsLaunch(args, s, coef, skip_ptr,
                                partials.data_ptr<float>(), stream));
    HIP_CHECK(LambTrustLaunch(args, partials.data_ptr<float>(), adapt,
                              skip_ptr, trust.data_ptr<float>(), stream));
    HIP_CHECK(LambUpdateLaunch(args, s, trust.data_ptr<float>(), skip_ptr,
                               stream));
    base += args.block_prefix[args.count];
  });
  for (int64_t i = 0; i < n; ++i) batch.Add(rows, (size_t)i, (unsigned int)i);
  batch.Flush();
  return trust;
}

at::Tensor FusedLarsStep(std::vector<at::Tensor>& params,
                         std::vector<at::Tensor>& grads,
                         std::vector<at::Tensor>& momenta, double lr,
                         double momentum, double weight_decay,
                         double trust_coefficient, double eps, bool nesterov,
                         bool trust_clip, bool adapt, at::Tensor grad_coef,
                         const std::vector<at::Tensor>* model_params,
                         at::Tensor skip) {
  Rows rows{&params, &grads, &momenta};
  const TupleInfo info = CheckTuples("fused_lars_step", "grads and momenta",
                                     rows, true, model_params);
  const int64_t n = (int64_t)params.size();
  c10::hip::HIPGuard guard(info.device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(info.device).stream();
  const float* coef = GradCoefPtr(grad_coef, info.device);
  const float* skip_ptr = SkipPtr(skip, info.device);
  auto f32 =
      at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, info.device);
  // sized for the whole call; every slot is written by exactly one block
  // before the trust kernel of its batch reads it
  at::Tensor partials =
      at::empty({std::max<int64_t>(2 * info.chunk_blocks, 1)}, f32);
  // empty tensors take no descriptor: their ratio is the preset 1
  at::Tensor trust = info.any_empty ? at::ones({n}, f32) : at::empty({n}, f32);
  LarsScalars s;
  s.lr = (float)lr;
  s.momentum = (float)momentum;
  s.weight_decay = (float)weight_decay;
  s.trust_coefficient = (float)trust_coefficient;
  s.eps = (float)eps;
  s.nesterov = nesterov;
  s.trust_clip = trust_clip;
  s.adapt = adapt;
  unsigned long long base = 0;
  if (model_params) {
    rows.push_back(model_params);
    ForEachMasterBatch<LarsMasterBatchArgs>(
        rows, true, [&](LarsMasterBatchArgs& args, int dt) {
          args.partial_base = base;
          HIP_CHECK(LarsNormsMasterLaunch(args, dt, coef, skip_ptr,
                                          partials.data_ptr<float>(), stream));
          HIP_CHECK(LarsTrustLaunch(args, s, partials.data_ptr<float>(),
                                    skip_ptr, trust.data_ptr<float>(),
                                    stream));
          HIP_CHECK(LarsUpdateMasterLaunch(args, dt, s, coef,
                                           trust.data_ptr<float>(), skip_ptr,
                                           stream));
          base += args.block_prefix[args.count];
        });
    return trust;
  }
  Batcher<LarsBatchArgs> batch([&](LarsBatchArgs& args) {
    args.partial_base = base;
    HIP_CHECK(LarsNormsLaunch(args, coef, skip_ptr,
                              partials.data_ptr<float>(), stream));
    HIP_CHECK(LarsTrustLaunch(args, s, partials.data_ptr<float>(), skip_ptr,
                              trust.data_ptr<float>(), stream));
    HIP_CHECK(LarsUpdateLaunch(args, s, coef, trust.data_ptr<float>(),
                               skip_ptr, stream));
    base += args.block_prefix[args.count];
  });
  for (int64_t i = 0; i < n; ++i) batch.Add(rows, (size_t)i, (unsigned int)i);
  batch.Flush();
  return trust;
}

}  // namespace gpu
}  // namespace hvd
