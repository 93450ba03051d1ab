// Device-side pieces shared by the BatchNorm kernel TUs (bn_kernels.hip,
// syncbn_kernels.hip): dtype conversion, 8-element vector access, and the
// fixed-channel 8-wide ("cl-vec8") decomposition of channels_last
// activations with C % 8 == 0: grid sizing, per-channel parameter loads and
// the reduction tail.  Included from .hip files only.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace hvd {
namespace gpu {
namespace {

template <typename T>
__device__ __forceinline__ float to_f(T v) { return (float)v; }
template <>
__device__ __forceinline__ float to_f<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <typename T>
__device__ __forceinline__ T from_f(float v) { return (T)v; }
template <>
__device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

// The fused BN+ReLU pre-activation gamma * xhat + beta of one element.  The
// forward stores relu of it, and the backward passes that do not read y
// recompute it to learn the ReLU mask, so it has to come out bit-identical
// in every kernel: each rounding step is spelled out, which leaves the
// compiler no contraction choice that could differ between them.
__device__ __forceinline__ float bn_preact(float x, float mean, float invstd,
                                           float gamma, float beta) {
  return fmaf(__fmul_rn(__fsub_rn(x, mean), invstd), gamma, beta);
}

// y > 0 as the forward stored it for pre-activation f (no residual): the
// round trip through T matters, a positive fp32 f can round to a zero fp16 y
template <typename T>
__device__ __forceinline__ bool bn_relu_mask(float f) {
  return to_f<T>(from_f<T>(f)) > 0.f;
}

// 8 consecutive elements = one 16-B access for 2-byte types, two for fp32.
template <typename T>
union Vec8 {
  uint4 u[2];  // u[1] is used by 4-byte types only
  T e[8];
  __device__ Vec8() {}
};

template <typename T>
__device__ __forceinline__ void load8(Vec8<T>& v, const T* p, long long i) {
  if (sizeof(T) == 2) {
    v.u[0] = ((const uint4*)p)[i];
  } else {
    v.u[0] = ((const uint4*)p)[i * 2];
    v.u[1] = ((const uint4*)p)[i * 2 + 1];
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, long long i, const Vec8<T>& v) {
  if (sizeof(T) == 2) {
    ((uint4*)p)[i] = v.u[0];
  } else {
    ((uint4*)p)[i * 2] = v.u[0];
    ((uint4*)p)[i * 2 + 1] = v.u[1];
  }
}

inline int grid_for(long long total, int C, int vecs_per_thread = 1) {
  // vecs_per_thread > 1 for the REDUCTION kernels: their per-block flush
  // costs 2*C global atomicAdds, so wide-channel shapes with few rows must
  // amortize it over more elements per block (measured: at C=2048, N*H*W
  // = 3136 the old 1-vec grid issued ~1.3 atomics PER ELEMENT and lost
  // ~40% to MIOpen; 8 vecs/thread cuts the flush traffic 8x).  Elementwise
  // kernels keep 1 for maximum bandwidth-filling parallelism.
  long long blocks = (total / 8 + 256LL * vecs_per_thread - 1) /
                     (256LL * vecs_per_thread);
  blocks = std::min<long long>(blocks > 0 ? blocks : 1, 2048);
  // fixed-channel decomposition invariant: (blocks*256*8) % C == 0 so each
  // thread's channel octet is stride-invariant.  vecs_per_row = C/8 <= 512;
  // round blocks up to a multiple of ceil(C/8/256) and ensure divisibility.
  long long vpr = C / 8;  // vectors per row
  long long g = std::__gcd((long long)256, vpr);
  long long mult = vpr / g;  // blocks must be a multiple of this
  blocks = ((blocks + mult - 1) / mult) * mult;
  return (int)blocks;
}

// cl-vec8: the 8 per-channel values of a thread's octet as two 16-B loads
// (the launcher checks that every parameter array is 16-B aligned); a null
// array reads as `fill`.
__device__ __forceinline__ void load_octet(float (&r)[8], const float* p,
                                           int c0, float fill) {
  if (p) {
    const float4 lo = *(const float4*)(p + c0);
    const float4 hi = *(const float4*)(p + c0 + 4);
    r[0] = lo.x; r[1] = lo.y; r[2] = lo.z; r[3] = lo.w;
    r[4] = hi.x; r[5] = hi.y; r[6] = hi.z; r[7] = hi.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = fill;
  }
}

// first channel of the calling thread's octet; the grid has fewer than 2^31
// threads and (threads * 8) % C == 0, so it is the same for every vector
// the thread visits
__device__ __forceinline__ int octet_channel(int C) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  return (int)(t % (unsigned)(C / 8)) * 8;
}

// cl-vec8 reduction tail: a thread's 2 x 8 partials of its channel octet ->
// the block's LDS bins [2C] (zeroed, barrier passed) -> one atomicAdd per
// (block, channel) into bank blockIdx % kBnBanks of [2C] floats.  When C/8
// is a power of two below 64, lanes l and l ^ o of a wave hold the same
// octet for every o that is a multiple of C/8: those fold by shuffle first,
// so C/8 lanes per wave touch LDS instead of 64 colliding ones.
__device__ __forceinline__ void octet_flush(float (&a)[8], float (&b)[8],
                                            int c0, int C, float* lds,
                                            float* __restrict__ banks) {
  const int vpr = C / 8;
  bool owner = true;
  if (vpr < 64 && (vpr & (vpr - 1)) == 0) {
    for (int o = 32; o >= vpr; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        a[k] += __shfl_xor(a[k], o, 64);
        b[k] += __shfl_xor(b[k], o, 64);
      }
    }
    owner = (int)(threadIdx.x & 63) < vpr;
  }
  if (owner) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      atomicAdd(&lds[c0 + k], a[k]);
      atomicAdd(&lds[C + c0 + k], b[k]);
    }
  }
  __syncthreads();
  float* bank = banks + (size_t)(blockIdx.x & (kBnBanks - 1)) * 2 * C;
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x)
    if (lds[c] != 0.f) atomicAdd(&bank[c], lds[c]);
}

// Grid of a cl-vec8 reduction.  Every block flushes 2C float atomics, and
// measured on MI355X that flush, not the read, set the time of wide-C
// shapes (64x512x28x28 bf16: 50 us at 1568 blocks against 14 us for the
// planar kernel on the same bytes).  So on top of grid_for's 8 vectors per
// thread the grid is capped at 2^18 flushed floats in all, but not below one
// block per CU; the kernels keep several loads in flight per thread to make
// up for the smaller grid.
inline int vec8_reduce_grid(long long total, int C) {
  const long long nvec = total / 8;
  const long long max_blocks = std::max<long long>(256, (1LL << 17) / C);
  long long vpt = (nvec + 256 * max_blocks - 1) / (256 * max_blocks);
  return grid_for(total, C, (int)std::max<long long>(8, vpt));
}

inline bool aligned_to(const void* const* ptrs, int n, size_t a) {
  for (int i = 0; i < n; ++i)
    if (ptrs[i] && ((uintptr_t)ptrs[i] % a) != 0) return false;
  return true;
}

}  // namespace
}  // namespace gpu
}  // namespace hvd
