// Device-side pieces shared by the kernel TUs that keep a row of H elements in
// the registers of one, two or four waves (ln_kernels.hip, emb_kernels.hip):
// the block shape, parameter loads, the row reduction and the dispatch over
// dtype and row length.  Included from .hip files only.
#pragma once

#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kLnThreads = 256;
constexpr int kLnWaves = kLnThreads / 64;

// The 8 parameter values of vector vi: fp32 (two 16-B loads) or T; a null
// array reads as `fill`.
template <typename T>
__device__ __forceinline__ void ln_param8(float (&r)[8], const void* p,
                                          bool f32, int vi, float fill) {
  if (!p) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = fill;
  } else if (f32 || sizeof(T) == 4) {
    const float4 lo = ((const float4*)p)[vi * 2];
    const float4 hi = ((const float4*)p)[vi * 2 + 1];
    r[0] = lo.x; r[1] = lo.y; r[2] = lo.z; r[3] = lo.w;
    r[4] = hi.x; r[5] = hi.y; r[6] = hi.z; r[7] = hi.w;
  } else {
    Vec8<T> v;
    load8(v, (const T*)p, vi);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = to_f<T>(v.e[k]);
  }
}

// Sum of v over the WPR waves that share a row, in every lane of them.  With
// WPR > 1 every thread of the block has to call it (two barriers); the waves'
// sums are added in rising wave order.
template <int WPR>
__device__ __forceinline__ float ln_row_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (WPR == 1) return v;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  const int base = wave / WPR * WPR;
  float s = red[base];
#pragma unroll
  for (int k = 1; k < WPR; ++k) s += red[base + k];
  __syncthreads();
  return s;
}

#define LN_DISPATCH_T(DT, ...)                                          \
  switch (DT) {                                                         \
    case DT_F32: { using scalar_t = float; __VA_ARGS__; break; }        \
    case DT_F16: { using scalar_t = __half; __VA_ARGS__; break; }       \
    case DT_BF16: { using scalar_t = __hip_bfloat16; __VA_ARGS__; break; } \
    default: return hipErrorInvalidValue;                               \
  }

// vectors per lane and waves per row for rows of H elements
#define LN_DISPATCH_H(H, ...)                                        \
  if ((H) <= 512) { constexpr int NV = 1, WPR = 1; __VA_ARGS__; }    \
  else if ((H) <= 1024) { constexpr int NV = 2, WPR = 1; __VA_ARGS__; } \
  else if ((H) <= 2048) { constexpr int NV = 2, WPR = 2; __VA_ARGS__; } \
  else { constexpr int NV = 2, WPR = 4; __VA_ARGS__; }

#define LN_DISPATCH_B(B, NAME, ...)                       \
  if (B) { constexpr bool NAME = true; __VA_ARGS__; }     \
  else { constexpr bool NAME = false; __VA_ARGS__; }

inline int ln_waves_per_row(int H) {
  return H <= 1024 ? 1 : (H <= 2048 ? 2 : 4);
}

}  // namespace
}  // namespace gpu
}  // namespace hvd
