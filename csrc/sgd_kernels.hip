// Fused SGD step for CDNA4: one launch updates every parameter bucket
// (momentum + weight decay + parameter update in a single HBM pass per
// tensor, instead of torch-eager's 3-4 kernels per parameter).
//
// Memory-bound: vectorized 16-byte accesses per lane, wave64, grid-stride
// within each (param, grad, momentum) triple; grid = count * blocks_per.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "kernels.h"
#include "multi_tensor.h"

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
  float* __restrict__ p = (float*)args.ptr[kRowParam][t];
  const float* __restrict__ g = (const float*)args.ptr[kRowGrad][t];
  float* __restrict__ m =
      HAS_MOMENTUM ? (float*)args.ptr[kRowMomentum][t] : nullptr;
  const long long n = (long long)args.numel[t];
  const long long tid =
      (long long)(blockIdx.x % blocks_per) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per * blockDim.x;

  long long done = 0;
  if (aligned16(p, g, m)) {  // m is null without momentum
    const long long nvec = n / 4;
    done = nvec * 4;
    for (long long i = tid; i < nvec; i += nthreads) {
      float4 pv = ((float4*)p)[i];
      float4 gv = ((const float4*)g)[i];
      float4 mv = HAS_MOMENTUM ? ((float4*)m)[i] : float4{0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        sgd_element<NESTEROV, HAS_MOMENTUM, HAS_COEF>(
            (&pv.x)[k], (&gv.x)[k], (&mv.x)[k], coef, lr, momentum,
            weight_decay, dampening);
      ((float4*)p)[i] = pv;
      if (HAS_MOMENTUM) ((float4*)m)[i] = mv;
    }
  }
  for (long long i = done + tid; i < n; i += nthreads) {
    float pe = p[i], me = HAS_MOMENTUM ? m[i] : 0.0f;
    sgd_element<NESTEROV, HAS_MOMENTUM, HAS_COEF>(pe, g[i], me, coef, lr,
                                                  momentum, weight_decay,
                                                  dampening);
    p[i] = pe;
    if (HAS_MOMENTUM) m[i] = me;
  }
}

template <bool NESTEROV, bool HAS_MOMENTUM>
void launch_sgd(const SgdBatchArgs& args, float lr, float momentum,
                float weight_decay, float dampening, const float* grad_coef,
                hipStream_t stream) {
  const int bpc = kBlocksPerTensor;
  dim3 grid(args.count * bpc), block(256);
  auto kernel = grad_coef ? fused_sgd_k<NESTEROV, HAS_MOMENTUM, true>
                          : fused_sgd_k<NESTEROV, HAS_MOMENTUM, false>;
  kernel<<<grid, block, 0, stream>>>(args, bpc, lr, momentum, weight_decay,
                                     dampening, grad_coef);
}

}  // namespace

hipError_t FusedSgdLaunch(const SgdBatchArgs& args, float lr, float momentum,
                          float weight_decay, float dampening, bool nesterov,
                          const float* grad_coef, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  auto launch = momentum == 0.0f ? launch_sgd<false, false>
                : nesterov       ? launch_sgd<true, true>
                                 : launch_sgd<false, true>;
  launch(args, lr, momentum, weight_decay, dampening, grad_coef, stream);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
