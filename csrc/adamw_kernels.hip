// Fused AdamW step for CDNA4: one launch updates every parameter bucket
// (exp_avg + exp_avg_sq + decoupled weight decay + parameter update in a
// single HBM pass per tensor — torch-eager AdamW issues ~8 kernels per
// parameter).  Beyond-parity MI355X feature (the reference fuses nothing);
// structure mirrors sgd_kernels.hip: 16-byte lanes, wave64, grid-stride
// within each tensor, grid = count * blocks_per.
//
// Bias correction is folded host-side into step_size = lr/bc1 and
// inv_bc2_sqrt = 1/sqrt(bc2); the per-element arithmetic is adamw_element
// in multi_tensor.h (torch AdamW definition, denom = sqrt(v)/sqrt(bc2) +
// eps).
//
// Master weights: the same kernel with a 2-byte gradient and a 2-byte model
// parameter row (LP, multi_tensor.h); fp32 and master-weight launches both
// move 28 bytes per element.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

template <typename LP>
using AdamwArgsOf = typename std::conditional<LowPrec<LP>::kModel,
                                              AdamwMasterBatchArgs,
                                              AdamwBatchArgs>::type;

template <typename LP, bool HAS_COEF>
__global__ __launch_bounds__(256) void fused_adamw_k(
    AdamwArgsOf<LP> args, int blocks_per, float lr, float beta1, float beta2,
    float eps, float weight_decay, float step_size, float inv_bc2_sqrt,
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
  float* __restrict__ m = (float*)args.ptr[kRowExpAvg][t];
  float* __restrict__ v = (float*)args.ptr[kRowExpAvgSq][t];
  G* __restrict__ q = nullptr;  // stays null without a model row
  if constexpr (MODEL) q = (G*)args.ptr[kRowModel][t];
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;
  const float decay = 1.0f - lr * weight_decay;

  long long done = 0;
  if (aligned16(p, g, m, v, q)) {
    const long long nvec = n / W;
    done = nvec * W;
    for (long long i = tid; i < nvec; i += nthreads) {
      float pv[W], gv[W], mv[W], vv[W];
      load_f32_vec(p, i, pv);
      load_grad_vec(g, i, gv);
      load_f32_vec(m, i, mv);
      load_f32_vec(v, i, vv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        adamw_element<HAS_COEF>(pv[k], gv[k], mv[k], vv[k], coef, beta1, beta2,
                                eps, decay, step_size, inv_bc2_sqrt);
      store_f32_vec(p, i, pv);
      store_f32_vec(m, i, mv);
      store_f32_vec(v, i, vv);
      if constexpr (MODEL) store_lp_vec(q, i, pv);
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    float pe = p[i], me = m[i], ve = v[i];
    adamw_element<HAS_COEF>(pe, (float)g[i], me, ve, coef, beta1, beta2, eps,
                            decay, step_size, inv_bc2_sqrt);
    p[i] = pe;
    m[i] = me;
    v[i] = ve;
    if constexpr (MODEL) q[i] = round_lp<G>(pe);
  }
}

template <typename LP>
hipError_t launch_adamw(const AdamwArgsOf<LP>& args, float lr, float beta1,
                        float beta2, float eps, float weight_decay,
                        long long step, const float* grad_coef,
                        const float* skip, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2 = 1.0f - powf(beta2, (float)step);
  const float step_size = lr / bc1;
  const float inv_bc2_sqrt = 1.0f / sqrtf(bc2);
  const int bpc = kBlocksPerTensor;
  dim3 grid(args.count * bpc), block(256);
  auto kernel = grad_coef ? fused_adamw_k<LP, true> : fused_adamw_k<LP, false>;
  kernel<<<grid, block, 0, stream>>>(args, bpc, lr, beta1, beta2, eps,
                                     weight_decay, step_size, inv_bc2_sqrt,
                                     grad_coef, skip);
  return hipGetLastError();
}

}  // namespace

hipError_t FusedAdamwLaunch(const AdamwBatchArgs& args, float lr, float beta1,
                            float beta2, float eps, float weight_decay,
                            long long step, const float* grad_coef,
                            const float* skip, hipStream_t stream) {
  return launch_adamw<void>(args, lr, beta1, beta2, eps, weight_decay, step,
                            grad_coef, skip, stream);
}

hipError_t FusedAdamwMasterLaunch(const AdamwMasterBatchArgs& args, int dt,
                                  float lr, float beta1, float beta2,
                                  float eps, float weight_decay,
                                  long long step, const float* grad_coef,
                                  const float* skip, hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_adamw<__half>(args, lr, beta1, beta2, eps, weight_decay,
                                  step, grad_coef, skip, stream);
    case DT_BF16:
      return launch_adamw<__hip_bfloat16>(args, lr, beta1, beta2, eps,
                                          weight_decay, step, grad_coef,
                                          skip, stream);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace gpu
}  // namespace hvd
