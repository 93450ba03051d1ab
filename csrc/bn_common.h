// Device-side pieces shared by the BatchNorm kernel TUs (bn_kernels.hip,
// syncbn_kernels.hip): dtype conversion, 8-element vector access and the
// fixed-channel grid sizing for channels_last activations with C % 8 == 0.
// Included from .hip files only.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <algorithm>

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

}  // namespace
}  // namespace gpu
}  // namespace hvd
