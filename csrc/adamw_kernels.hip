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
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

template <bool HAS_COEF>
__global__ __launch_bounds__(256) void fused_adamw_k(
    AdamwBatchArgs args, int blocks_per, float lr, float beta1, float beta2,
    float eps, float weight_decay, float step_size, float inv_bc2_sqrt,
    const float* __restrict__ grad_coef) {
  int t = blockIdx.x / blocks_per;
  if (t >= args.count) return;
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  float* __restrict__ p = (float*)args.ptr[kRowParam][t];
  const float* __restrict__ g = (const float*)args.ptr[kRowGrad][t];
  float* __restrict__ m = (float*)args.ptr[kRowExpAvg][t];
  float* __restrict__ v = (float*)args.ptr[kRowExpAvgSq][t];
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;
  const float decay = 1.0f - lr * weight_decay;

  long long done = 0;
  if (aligned16(p, g, m, v)) {
    const long long nvec = n / 4;
    done = nvec * 4;
    for (long long i = tid; i < nvec; i += nthreads) {
      float4 pv = ((float4*)p)[i];
      float4 gv = ((const float4*)g)[i];
      float4 mv = ((float4*)m)[i];
      float4 vv = ((float4*)v)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        adamw_element<HAS_COEF>((&pv.x)[k], (&gv.x)[k], (&mv.x)[k],
                                (&vv.x)[k], coef, beta1, beta2, eps, decay,
                                step_size, inv_bc2_sqrt);
      ((float4*)p)[i] = pv;
      ((float4*)m)[i] = mv;
      ((float4*)v)[i] = vv;
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    adamw_element<HAS_COEF>(p[i], g[i], m[i], v[i], coef, beta1, beta2, eps,
                            decay, step_size, inv_bc2_sqrt);
  }
}

}  // namespace

hipError_t FusedAdamwLaunch(const AdamwBatchArgs& args, float lr, float beta1,
                            float beta2, float eps, float weight_decay,
                            long long step, const float* grad_coef,
                            hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2 = 1.0f - powf(beta2, (float)step);
  const float step_size = lr / bc1;
  const float inv_bc2_sqrt = 1.0f / sqrtf(bc2);
  const int bpc = kBlocksPerTensor;
  dim3 grid(args.count * bpc), block(256);
  auto kernel = grad_coef ? fused_adamw_k<true> : fused_adamw_k<false>;
  kernel<<<grid, block, 0, stream>>>(args, bpc, lr, beta1, beta2, eps,
                                     weight_decay, step_size, inv_bc2_sqrt,
                                     grad_coef);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
