// Fused SGD step for CDNA4: one launch updates every parameter bucket
// (momentum + weight decay + parameter update in a single HBM pass per
// tensor, instead of torch-eager's 3-4 kernels per parameter).
//
// Memory-bound: vectorized 16-byte accesses per lane, wave64, grid-stride
// within each (param, grad, momentum) triple; grid = count * blocks_per.
//
// Master weights: the same kernel with a 2-byte gradient and a 2-byte model
// parameter row that receives the rounded master (LP, multi_tensor.h).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

template <typename LP>
using SgdArgsOf = typename std::conditional<LowPrec<LP>::kModel,
                                            SgdMasterBatchArgs,
                                            SgdBatchArgs>::type;

// LP: void, or the 2-byte type of the gradient and the model parameter
// (master weights, multi_tensor.h).
template <typename LP, bool NESTEROV, bool HAS_MOMENTUM, bool HAS_COEF>
__global__ __launch_bounds__(256) void fused_sgd_k(
    SgdArgsOf<LP> args, int blocks_per, float lr, float momentum,
    float weight_decay, float dampening,
    const float* __restrict__ grad_coef, const float* __restrict__ skip) {
  using G = typename LowPrec<LP>::Grad;
  constexpr bool MODEL = LowPrec<LP>::kModel;
  constexpr int W = LowPrec<LP>::kVec;
  // one uniform load: a set flag (an overflowed step) leaves every row as
  // it is
  if (skip && *skip != 0.0f) return;
  int t = blockIdx.x / blocks_per;
  if (t >= args.count) return;
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  float* __restrict__ p = (float*)args.ptr[kRowParam][t];
  const G* __restrict__ g = (const G*)args.ptr[kRowGrad][t];
  float* __restrict__ m =
      HAS_MOMENTUM ? (float*)args.ptr[kRowMomentum][t] : nullptr;
  G* __restrict__ q = nullptr;
  if constexpr (MODEL) q = (G*)args.ptr[kRowSgdModel][t];
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;

  long long done = 0;
  if (aligned16(p, g, m, q)) {  // m, q are null without momentum, model row
    const long long nvec = n / W;
    done = nvec * W;
    for (long long i = tid; i < nvec; i += nthreads) {
      float pv[W], gv[W], mv[W] = {};
      load_f32_vec(p, i, pv);
      load_grad_vec(g, i, gv);
      if (HAS_MOMENTUM) load_f32_vec(m, i, mv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        sgd_element<NESTEROV, HAS_MOMENTUM, HAS_COEF>(
            pv[k], gv[k], mv[k], coef, lr, momentum, weight_decay, dampening);
      store_f32_vec(p, i, pv);
      if (HAS_MOMENTUM) store_f32_vec(m, i, mv);
      if constexpr (MODEL) store_lp_vec(q, i, pv);
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    float pe = p[i], me = HAS_MOMENTUM ? m[i] : 0.0f;
    sgd_element<NESTEROV, HAS_MOMENTUM, HAS_COEF>(pe, (float)g[i], me, coef,
                                                  lr, momentum, weight_decay,
                                                  dampening);
    p[i] = pe;
    if (HAS_MOMENTUM) m[i] = me;
    if constexpr (MODEL) q[i] = round_lp<G>(pe);
  }
}

template <typename LP, bool NESTEROV, bool HAS_MOMENTUM>
void launch_sgd(const SgdArgsOf<LP>& args, float lr, float momentum,
                float weight_decay, float dampening, const float* grad_coef,
                const float* skip, hipStream_t stream) {
  const int bpc = kBlocksPerTensor;
  dim3 grid(args.count * bpc), block(256);
  auto kernel = grad_coef ? fused_sgd_k<LP, NESTEROV, HAS_MOMENTUM, true>
                          : fused_sgd_k<LP, NESTEROV, HAS_MOMENTUM, false>;
  kernel<<<grid, block, 0, stream>>>(args, bpc, lr, momentum, weight_decay,
                                     dampening, grad_coef, skip);
}

template <typename LP>
hipError_t launch_sgd_variant(const SgdArgsOf<LP>& args, float lr,
                              float momentum, float weight_decay,
                              float dampening, bool nesterov,
                              const float* grad_coef, const float* skip,
                              hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  auto launch = momentum == 0.0f ? launch_sgd<LP, false, false>
                : nesterov       ? launch_sgd<LP, true, true>
                                 : launch_sgd<LP, false, true>;
  launch(args, lr, momentum, weight_decay, dampening, grad_coef, skip,
         stream);
  return hipGetLastError();
}

}  // namespace

hipError_t FusedSgdLaunch(const SgdBatchArgs& args, float lr, float momentum,
                          float weight_decay, float dampening, bool nesterov,
                          const float* grad_coef, const float* skip,
                          hipStream_t stream) {
  return launch_sgd_variant<void>(args, lr, momentum, weight_decay, dampening,
                                  nesterov, grad_coef, skip, stream);
}

hipError_t FusedSgdMasterLaunch(const SgdMasterBatchArgs& args, int dt,
                                float lr, float momentum, float weight_decay,
                                float dampening, bool nesterov,
                                const float* grad_coef, const float* skip,
                                hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_sgd_variant<__half>(args, lr, momentum, weight_decay,
                                        dampening, nesterov, grad_coef,
                                        skip, stream);
    case DT_BF16:
      return launch_sgd_variant<__hip_bfloat16>(args, lr, momentum,
                                                weight_decay, dampening,
                                                nesterov, grad_coef, skip,
                                                stream);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace gpu
}  // namespace hvd
