// Fused AdamW step for CDNA4: one launch updates every parameter bucket
// (exp_avg + exp_avg_sq + decoupled weight decay + parameter update in a
// single HBM pass per tensor — torch-eager AdamW issues ~8 kernels per
// parameter).  Beyond-parity MI355X feature (the reference fuses nothing);
// structure mirrors sgd_kernels.hip: 16-byte lanes, wave64, grid-stride
// within each tensor, grid = count * blocks_per.
//
// Bias correction is folded host-side into step_size = lr/bc1 and
// inv_bc2_sqrt = 1/sqrt(bc2) so the kernel is pure FMA per element:
//   m = b1*m + (1-b1)*g
//   v = b2*v + (1-b2)*g*g
//   p = p*(1 - lr*wd) - step_size * m / (sqrt(v)*inv_bc2_sqrt... )
// using denom = sqrt(v)/sqrt(bc2) + eps (torch AdamW definition).
#include <hip/hip_runtime.h>

#include "grad_scale.h"
#include "kernels.h"

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
  float* __restrict__ p = (float*)args.params[t];
  const float* __restrict__ g = (const float*)args.grads[t];
  float* __restrict__ m = (float*)args.exp_avg[t];
  float* __restrict__ v = (float*)args.exp_avg_sq[t];
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;
  const float decay = 1.0f - lr * weight_decay;

  const bool vec_ok = (((uintptr_t)p & 15) == 0) &&
                      (((uintptr_t)g & 15) == 0) &&
                      (((uintptr_t)m & 15) == 0) &&
                      (((uintptr_t)v & 15) == 0);
  long long done = 0;
  if (vec_ok) {
    const long long nvec = n / 4;
    done = nvec * 4;
    for (long long i = tid; i < nvec; i += nthreads) {
      float4 pv = ((float4*)p)[i];
      float4 gv = ((const float4*)g)[i];
      float4 mv = ((float4*)m)[i];
      float4 vv = ((float4*)v)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float ge = (&gv.x)[k];
        if (HAS_COEF) ge = scale_grad(ge, coef);
        float me = beta1 * (&mv.x)[k] + (1.0f - beta1) * ge;
        float ve = beta2 * (&vv.x)[k] + (1.0f - beta2) * ge * ge;
        (&mv.x)[k] = me;
        (&vv.x)[k] = ve;
        float denom = sqrtf(ve) * inv_bc2_sqrt + eps;
        (&pv.x)[k] = (&pv.x)[k] * decay - step_size * me / denom;
      }
      ((float4*)p)[i] = pv;
      ((float4*)m)[i] = mv;
      ((float4*)v)[i] = vv;
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    float ge = g[i];
    if (HAS_COEF) ge = scale_grad(ge, coef);
    float me = beta1 * m[i] + (1.0f - beta1) * ge;
    float ve = beta2 * v[i] + (1.0f - beta2) * ge * ge;
    m[i] = me;
    v[i] = ve;
    float denom = sqrtf(ve) * inv_bc2_sqrt + eps;
    p[i] = p[i] * decay - step_size * me / denom;
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
  const int bpc = 16;
  dim3 grid(args.count * bpc), block(256);
  if (grad_coef)
    fused_adamw_k<true><<<grid, block, 0, stream>>>(
        args, bpc, lr, beta1, beta2, eps, weight_decay, step_size,
        inv_bc2_sqrt, grad_coef);
  else
    fused_adamw_k<false><<<grid, block, 0, stream>>>(
        args, bpc, lr, beta1, beta2, eps, weight_decay, step_size,
        inv_bc2_sqrt, nullptr);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
