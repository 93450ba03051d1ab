// Device side shared by the multi-tensor kernels (clip, sgd, adamw, lamb and
// lars_kernels.hip): the chunked work division and fixed-order block sum of
// clip, LAMB and LARS, and the per-element arithmetic of every optimizer kernel,
// stated once and called from the kernel's 16-byte loop and its tail loop.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

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

// x as a value of its own: the empty asm keeps the compiler from fusing the
// operation that made it into a later one.
__device__ __forceinline__ float pinned(float x) {
  asm("" : "+v"(x));
  return x;
}

// ---- master weights ----------------------------------------------------------
// The optimizer kernels are templates on LP, the 2-byte type of the model
// parameter and its gradient (__half or __hip_bfloat16), or void for fp32
// parameters.  With LP the fp32 rows hold the master and the moments, the
// gradient is widened exactly as it is read, and the updated master also
// goes, rounded to nearest-even, to the model-parameter row.  The 16-byte
// loop then takes 8 elements per lane: one 16-byte access on each 2-byte row,
// two on each fp32 row.
template <typename LP>
struct LowPrec {
  static constexpr bool kModel = true;
  static constexpr int kVec = 8;  // elements per lane in the 16-byte loop
  using Grad = LP;
};
template <>
struct LowPrec<void> {
  static constexpr bool kModel = false;
  static constexpr int kVec = 4;
  using Grad = float;  // also the placeholder type of the absent model row
};

// x[0..W) = base[i * W ...] as W / 4 16-byte loads, and the matching store.
template <int W>
__device__ __forceinline__ void load_f32_vec(const float* base, long long i,
                                             float (&x)[W]) {
#pragma unroll
  for (int q = 0; q < W / 4; ++q) {
    const float4 v = ((const float4*)base)[i * (W / 4) + q];
    x[4 * q] = v.x;
    x[4 * q + 1] = v.y;
    x[4 * q + 2] = v.z;
    x[4 * q + 3] = v.w;
  }
}
template <int W>
__device__ __forceinline__ void store_f32_vec(float* base, long long i,
                                              const float (&x)[W]) {
#pragma unroll
  for (int q = 0; q < W / 4; ++q)
    ((float4*)base)[i * (W / 4) + q] =
        float4{x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
}
// The same for 8 values of a 2-byte type in one 16-byte access: widening is
// exact, the store rounds to nearest-even.  round_lp converts a value that
// has also been stored as fp32: pinned first, since an fma fused with the
// conversion would round once, from the exact result, and the model
// parameter would not be the rounded master.
template <typename T>
__device__ __forceinline__ T round_lp(float x) {
  return (T)pinned(x);
}
template <typename T>
__device__ __forceinline__ void load_lp_vec(const T* base, long long i,
                                            float (&x)[8]) {
  static_assert(sizeof(T) == 2, "fp16 or bf16");
  union {
    uint4 u;
    T e[8];
  } in;
  in.u = ((const uint4*)base)[i];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (float)in.e[k];
}
// 4 values of a 2-byte type in one 8-byte load (LARS' norm pass, which takes
// 4 elements per lane whatever the gradient's type).
template <typename T>
__device__ __forceinline__ void load_lp_quad(const T* base, long long i,
                                             float (&x)[4]) {
  static_assert(sizeof(T) == 2, "fp16 or bf16");
  union {
    uint2 u;
    T e[4];
  } in;
  in.u = ((const uint2*)base)[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = (float)in.e[k];
}
template <typename T>
__device__ __forceinline__ void store_lp_vec(T* base, long long i,
                                             const float (&x)[8]) {
  static_assert(sizeof(T) == 2, "fp16 or bf16");
  union {
    uint4 u;
    T e[8];
  } out;
#pragma unroll
  for (int k = 0; k < 8; ++k) out.e[k] = round_lp<T>(x[k]);
  ((uint4*)base)[i] = out.u;
}
// A gradient row: fp32 (W = 4) or 2-byte (W = 8).
template <typename G, int W>
__device__ __forceinline__ void load_grad_vec(const G* base, long long i,
                                              float (&x)[W]) {
  if constexpr (std::is_same<G, float>::value)
    load_f32_vec(base, i, x);
  else
    load_lp_vec(base, i, x);
}

// ---- per-element arithmetic -------------------------------------------------

// The fused multiply-adds below are written out.  Left to contraction, a sum
// of two products may have either one fused, and the compiler chooses
// differently from one loop or instantiation to the next; stated as fmaf the
// 16-byte loop and the tail loop of every instantiation (fp32, fp16, bf16)
// compute the same bits, those of the fp32 16-byte loops before there were
// others.

// g * coef, never contracted into the weight-decay add or the moment
// updates, so a clip coefficient of exactly 1 reproduces the unclipped
// update bit for bit.
__device__ __forceinline__ float scale_grad(float g, float coef) {
  return pinned(g * coef);
}

// torch.optim.SGD: weight decay into the gradient, momentum buffer, update.
template <bool NESTEROV, bool HAS_MOMENTUM, bool HAS_COEF>
__device__ __forceinline__ void sgd_element(float& p, float g, float& m,
                                            float coef, float lr,
                                            float momentum, float weight_decay,
                                            float dampening) {
  if (HAS_COEF) g = scale_grad(g, coef);
  g = fmaf(weight_decay, p, g);
  if (HAS_MOMENTUM) {
    m = fmaf(momentum, m, (1.0f - dampening) * g);
    g = NESTEROV ? fmaf(momentum, m, g) : m;
  }
  p = fmaf(-lr, g, p);
}

// Adam's two moments (AdamW and LAMB).
__device__ __forceinline__ void adam_moments(float& m, float& v, float g,
                                             float beta1, float beta2) {
  m = fmaf(1.0f - beta1, g, beta1 * m);
  v = fmaf((1.0f - beta2) * g, g, beta2 * v);
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
  const float denom = fmaf(sqrtf(ve), inv_bc2_sqrt, eps);
  p = fmaf(p, decay, -(step_size * me / denom));
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
  p = fmaf(-step, lamb_u(p, m, v, s), p);
}

// LARS pass 1: p^2 and g'^2 into the caller's accumulators.
template <bool HAS_COEF>
__device__ __forceinline__ void lars_norms_element(float p, float g,
                                                   float coef, float& pp,
                                                   float& gg) {
  if (HAS_COEF) g = scale_grad(g, coef);
  pp = fmaf(p, p, pp);
  gg = fmaf(g, g, gg);
}

// LARS pass 3: momentum SGD on d = trust * (g' + weight_decay * p).  d is
// pinned, so a trust ratio of exactly 1 (a no-decay group) gives the bits of
// sgd_element with dampening 0 on a buffer that starts at zero.
template <bool NESTEROV, bool HAS_COEF>
__device__ __forceinline__ void lars_element(float& p, float g, float& m,
                                             float coef, float trust,
                                             float lr, float momentum,
                                             float weight_decay) {
  if (HAS_COEF) g = scale_grad(g, coef);
  const float d = pinned(trust * fmaf(weight_decay, p, g));
  const float me = fmaf(momentum, m, d);  // m may be memory: one store
  m = me;
  p = fmaf(-lr, NESTEROV ? fmaf(momentum, me, d) : me, p);
}

}  // namespace gpu
}  // namespace hvd
