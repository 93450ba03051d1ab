// Device side shared by the multi-tensor kernels (clip, sgd, adamw and
// lamb_kernels.hip): the chunked work division and fixed-order block sum of
// clip and LAMB, and the per-element arithmetic of every optimizer kernel,
// stated once and called from the kernel's 16-byte loop and its tail loop.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace hvd {
namespace gpu {

// Block size of the chunked kernels: 8 float4 per thread and chunk.
constexpr int kChunkThreads = 256;
// Blocks per descriptor of the kernels that divide work per tensor (SGD,
// AdamW), each grid-striding over its tensor.
constexpr int kBlocksPerTensor = 16;

struct ChunkRef {
  int tensor;
  long long begin;  // element range of this block within the tensor
  long long end;
};

// Largest t with block_prefix[t] <= blockIdx.x (block_prefix[count] is the
// grid size, so the invariant prefix[lo] <= b < prefix[hi] always holds).
// Args: a chunked MultiTensorArgs.
template <typename Args>
__device__ __forceinline__ ChunkRef find_chunk(const Args& args) {
  const unsigned int b = blockIdx.x;
  int lo = 0, hi = args.count;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (args.block_prefix[mid] <= b) lo = mid; else hi = mid;
  }
  ChunkRef c;
  c.tensor = lo;
  c.begin = (long long)(b - args.block_prefix[lo]) * kChunkElems;
  const long long n = (long long)args.numel[lo];
  c.end = c.begin + kChunkElems < n ? c.begin + kChunkElems : n;
  return c;
}

// Sum over the block in a fixed order: wave64 shuffle tree, then the wave
// leaders through LDS.  Valid in thread 0.
__device__ __forceinline__ float block_sum(float v) {
  __shared__ float wave_part[kChunkThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  float total = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kChunkThreads / 64; ++w) total += wave_part[w];
  }
  return total;
}

// True when every pointer is 16-byte aligned (float4 access is allowed).
template <typename... P>
__device__ __forceinline__ bool aligned16(const P*... p) {
  return ((... | (uintptr_t)p) & 15) == 0;
}

// ---- per-element arithmetic -------------------------------------------------

// g * coef as a value of its own: the empty asm keeps the compiler from
// contracting the product into a later fma (the weight-decay add, the
// moment updates), so a clip coefficient of exactly 1 reproduces the
// unclipped update bit for bit.
__device__ __forceinline__ float scale_grad(float g, float coef) {
  float r = g * coef;
  asm("" : "+v"(r));
  return r;
}

// torch.optim.SGD: weight decay into the gradient, momentum buffer, update.
template <bool NESTEROV, bool HAS_MOMENTUM, bool HAS_COEF>
__device__ __forceinline__ void sgd_element(float& p, float g, float& m,
                                            float coef, float lr,
                                            float momentum, float weight_decay,
                                            float dampening) {
  if (HAS_COEF) g = scale_grad(g, coef);
  g += weight_decay * p;
  if (HAS_MOMENTUM) {
    m = momentum * m + (1.0f - dampening) * g;
    g = NESTEROV ? g + momentum * m : m;
  }
  p = p - lr * g;
}

// Adam's two moments (AdamW and LAMB).
__device__ __forceinline__ void adam_moments(float& m, float& v, float g,
                                             float beta1, float beta2) {
  m = beta1 * m + (1.0f - beta1) * g;
  v = beta2 * v + (1.0f - beta2) * g * g;
}

// torch.optim.AdamW with the bias correction folded on the host: decay =
// 1 - lr * weight_decay, step_size = lr / bc1, inv_bc2_sqrt = 1 / sqrt(bc2).
template <bool HAS_COEF>
__device__ __forceinline__ void adamw_element(float& p, float g, float& m,
                                              float& v, float coef,
                                              float beta1, float beta2,
                                              float eps, float decay,
                                              float step_size,
                                              float inv_bc2_sqrt) {
  if (HAS_COEF) g = scale_grad(g, coef);
  // m, v and p may be memory (the tail loops): one load and one store each
  float me = m, ve = v;
  adam_moments(me, ve, g, beta1, beta2);
  m = me;
  v = ve;
  const float denom = sqrtf(ve) * inv_bc2_sqrt + eps;
  p = p * decay - step_size * me / denom;
}

// LAMB's u from the already-updated moments.
__device__ __forceinline__ float lamb_u(float p, float m, float v,
                                        const LambScalars& s) {
  const float denom = sqrtf(v) * s.inv_bc2_sqrt + s.eps;
  return (m * s.inv_bc1) / denom + s.weight_decay * p;
}

// LAMB pass 1: moments in place, p^2 and u^2 into the caller's accumulators.
template <bool HAS_COEF>
__device__ __forceinline__ void lamb_moments_element(float p, float g,
                                                     float& m, float& v,
                                                     float coef,
                                                     const LambScalars& s,
                                                     float& pp, float& uu) {
  if (HAS_COEF) g = scale_grad(g, coef);
  float me = m, ve = v;  // as in adamw_element
  adam_moments(me, ve, g, s.beta1, s.beta2);
  m = me;
  v = ve;
  const float u = lamb_u(p, me, ve, s);
  pp += p * p;
  uu += u * u;
}

// LAMB pass 3: step = lr * trust ratio of the tensor.
__device__ __forceinline__ void lamb_update_element(float& p, float m, float v,
                                                    float step,
                                                    const LambScalars& s) {
  p = p - step * lamb_u(p, m, v, s);
}

}  // namespace gpu
}  // namespace hvd
