// Fused SGD step for CDNA4: one launch updates every parameter bucket
// (momentum + weight decay + parameter update in a single HBM pass per
// tensor, instead of torch-eager's 3-4 kernels per parameter).
//
// Memory-bound: vectorized 16-byte accesses per lane, wave64, grid-stride
// within each (param, grad, momentum) triple; grid = count * blocks_per.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "grad_scale.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

template <bool NESTEROV, bool HAS_MOMENTUM, bool HAS_COEF>
__global__ __launch_bounds__(256) void fused_sgd_k(
    SgdBatchArgs args, int blocks_per, float lr, float momentum,
    float weight_decay, float dampening,
    const float* __restrict__ grad_coef) {
  int t = blockIdx.x / blocks_per;
  if (t >= args.count) return;
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  float* __restrict__ p = (float*)args.params[t];
  const float* __restrict__ g = (const float*)args.grads[t];
  float* __restrict__ m = HAS_MOMENTUM ? (float*)args.momenta[t] : nullptr;
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;

  const bool vec_ok = (((uintptr_t)p & 15) == 0) && (((uintptr_t)g & 15) == 0) &&
                      (!HAS_MOMENTUM || ((uintptr_t)m & 15) == 0);
  long long done = 0;
  if (vec_ok) {
    const long long nvec = n / 4;
    done = nvec * 4;
    for (long long i = tid; i < nvec; i += nthreads) {
      float4 pv = ((float4*)p)[i];
      float4 gv = ((const float4*)g)[i];
      float4 mv = HAS_MOMENTUM ? ((float4*)m)[i] : float4{0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pe = (&pv.x)[k], ge = (&gv.x)[k];
        if (HAS_COEF) ge = scale_grad(ge, coef);
        ge += weight_decay * pe;
        if (HAS_MOMENTUM) {
          float me = momentum * (&mv.x)[k] + (1.0f - dampening) * ge;
          (&mv.x)[k] = me;
          ge = NESTEROV ? ge + momentum * me : me;
        }
        (&pv.x)[k] = pe - lr * ge;
      }
      ((float4*)p)[i] = pv;
      if (HAS_MOMENTUM) ((float4*)m)[i] = mv;
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    float pe = p[i], ge = g[i];
    if (HAS_COEF) ge = scale_grad(ge, coef);
    ge += weight_decay * pe;
    if (HAS_MOMENTUM) {
      float me = momentum * m[i] + (1.0f - dampening) * ge;
      m[i] = me;
      ge = NESTEROV ? ge + momentum * me : me;
    }
    p[i] = pe - lr * ge;
  }
}

template <bool NESTEROV, bool HAS_MOMENTUM>
void launch_sgd(const SgdBatchArgs& args, float lr, float momentum,
                float weight_decay, float dampening, const float* grad_coef,
                hipStream_t stream) {
  const int bpc = 16;
  dim3 grid(args.count * bpc), block(256);
  if (grad_coef)
    fused_sgd_k<NESTEROV, HAS_MOMENTUM, true><<<grid, block, 0, stream>>>(
        args, bpc, lr, momentum, weight_decay, dampening, grad_coef);
  else
    fused_sgd_k<NESTEROV, HAS_MOMENTUM, false><<<grid, block, 0, stream>>>(
        args, bpc, lr, momentum, weight_decay, dampening, nullptr);
}

}  // namespace

hipError_t FusedSgdLaunch(const SgdBatchArgs& args, float lr, float momentum,
                          float weight_decay, float dampening, bool nesterov,
                          const float* grad_coef, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  if (momentum != 0.0f) {
    if (nesterov)
      launch_sgd<true, true>(args, lr, momentum, weight_decay, dampening,
                             grad_coef, stream);
    else
      launch_sgd<false, true>(args, lr, momentum, weight_decay, dampening,
                              grad_coef, stream);
  } else {
    launch_sgd<false, false>(args, lr, momentum, weight_decay, dampening,
                             grad_coef, stream);
  }
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
