// Fused dropout + residual add + LayerNorm for the BERT encoder:
// y = LayerNorm(residual + dropout(x)) over rows of H contiguous elements.
//
// A row lives in registers.  Lane l of a wave holds the 8-element vectors
// l, l + 64 * WPR, ... of its row, at most two of them: rows up to 1024
// elements take one wave (WPR = 1), rows up to 2048 two and rows up to 4096
// all four waves of the block, which then meet through a few LDS words.  So
// the register count does not grow with H, x and residual are read once, and
// the variance comes from the centred values (mean first, then
// sum((z - mean)^2)): residual streams carry a large mean, which E[z^2] -
// mean^2 would cancel against.
//
// Backward is one pass over dy and z that writes dz (and dx = dz * keep *
// scale under dropout) and, for the parameter gradients, one partial row of
// [2H] per block, plus a small kernel that folds the partial rows in a fixed
// order.  No atomics anywhere: identical inputs give identical bits.
//
// The dropout mask is recomputed from (seed, offset, vector index) by
// ln_keep8 (ln_philox.h) wherever it is needed and never stored.
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

// Block b takes the row groups b, b + gridDim.x, ...; a group is the
// kLnWaves / WPR rows the block holds at a time.  Vector i of a lane is
// vector (i * WPR + wave % WPR) * 64 + lane of the row.
template <typename T, int NV, int WPR, bool DROP>
__global__ __launch_bounds__(kLnThreads) void ln_fwd_k(
    const T* __restrict__ x, const T* __restrict__ res,
    const void* __restrict__ gamma, bool gamma_f32,
    const void* __restrict__ beta, bool beta_f32, T* __restrict__ y,
    T* __restrict__ z, float* __restrict__ mean, float* __restrict__ rstd,
    long long M, int H, float eps, LnDropout d) {
  __shared__ float red[kLnWaves];
  constexpr int RPB = kLnWaves / WPR;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int vpr = H / 8;
  const float inv_h = 1.0f / (float)H;
  const long long groups = (M + RPB - 1) / RPB;
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long long row = g * RPB + wave / WPR;
    const bool live = row < M;
    float zf[NV][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = (i * WPR + wave % WPR) * 64 + lane;
      if (live && vi < vpr) {
        const long long v = row * vpr + vi;
        Vec8<T> xv;
        load8(xv, x, v);
        float r[8];
        if (res) {
          Vec8<T> rv;
          load8(rv, res, v);
#pragma unroll
          for (int k = 0; k < 8; ++k) r[k] = to_f<T>(rv.e[k]);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) r[k] = 0.f;
        }
        unsigned int keep = 0xFFu;
        if (DROP) keep = ln_keep8(d, (unsigned long long)v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float a = to_f<T>(xv.e[k]);
          if (DROP) a = ((keep >> k) & 1u) ? a * d.scale : 0.f;
          zf[i][k] = r[k] + a;
          s += zf[i][k];
        }
        if (z) {
          Vec8<T> zv;
#pragma unroll
          for (int k = 0; k < 8; ++k) zv.e[k] = from_f<T>(zf[i][k]);
          store8(z, v, zv);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) zf[i][k] = 0.f;
      }
    }
    const float m = ln_row_sum<WPR>(s, red) * inv_h;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = (i * WPR + wave % WPR) * 64 + lane;
      if (vi < vpr) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float c = zf[i][k] - m;
          q += c * c;
        }
      }
    }
    const float rs = rsqrtf(ln_row_sum<WPR>(q, red) * inv_h + eps);
    if (live && lane == 0 && wave % WPR == 0) {
      mean[row] = m;
      rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = (i * WPR + wave % WPR) * 64 + lane;
      if (live && vi < vpr) {
        float ga[8], be[8];
        ln_param8<T>(ga, gamma, gamma_f32, vi, 1.f);
        ln_param8<T>(be, beta, beta_f32, vi, 0.f);
        Vec8<T> yv;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          yv.e[k] = from_f<T>((zf[i][k] - m) * rs * ga[k] + be[k]);
        store8(y, row * vpr + vi, yv);
      }
    }
  }
}

// WG: also accumulate sum(dy * xhat) and sum(dy) per column over the rows
// this block visits, in registers, and write them as partial row blockIdx.x
// of [2H].  The waves that own the same columns (one per row of the group)
// meet in the dynamic LDS [2H], added in rising wave order.
template <typename T, int NV, int WPR, bool DROP, bool WG>
__global__ __launch_bounds__(kLnThreads) void ln_bwd_k(
    const T* __restrict__ dy, const T* __restrict__ z,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const void* __restrict__ gamma, bool gamma_f32, T* __restrict__ dz,
    T* __restrict__ dx, float* __restrict__ partials, long long M, int H,
    LnDropout d) {
  extern __shared__ float4 ln_lds[];
  __shared__ float red[kLnWaves];
  constexpr int RPB = kLnWaves / WPR;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int vpr = H / 8;
  const float inv_h = 1.0f / (float)H;
  const long long groups = (M + RPB - 1) / RPB;
  float ag[NV][8], ab[NV][8];
  if (WG) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) ag[i][k] = ab[i][k] = 0.f;
  }
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long long row = g * RPB + wave / WPR;
    const bool live = row < M;
    const float m = live ? mean[row] : 0.f;
    const float rs = live ? rstd[row] : 0.f;
    float xh[NV][8], gg[NV][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = (i * WPR + wave % WPR) * 64 + lane;
      if (live && vi < vpr) {
        const long long v = row * vpr + vi;
        Vec8<T> dv, zv;
        load8(dv, dy, v);
        load8(zv, z, v);
        float ga[8];
        ln_param8<T>(ga, gamma, gamma_f32, vi, 1.f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float dyk = to_f<T>(dv.e[k]);
          xh[i][k] = (to_f<T>(zv.e[k]) - m) * rs;
          gg[i][k] = dyk * ga[k];
          s1 += gg[i][k];
          s2 += gg[i][k] * xh[i][k];
          if (WG) {
            ag[i][k] += dyk * xh[i][k];
            ab[i][k] += dyk;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) xh[i][k] = gg[i][k] = 0.f;
      }
    }
    const float a = ln_row_sum<WPR>(s1, red) * inv_h;
    const float b = ln_row_sum<WPR>(s2, red) * inv_h;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = (i * WPR + wave % WPR) * 64 + lane;
      if (live && vi < vpr) {
        const long long v = row * vpr + vi;
        float dzf[8];
        Vec8<T> ov;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          dzf[k] = rs * (gg[i][k] - a - xh[i][k] * b);
          ov.e[k] = from_f<T>(dzf[k]);
        }
        store8(dz, v, ov);
        if (DROP) {
          const unsigned int keep = ln_keep8(d, (unsigned long long)v);
#pragma unroll
          for (int k = 0; k < 8; ++k)
            ov.e[k] =
                from_f<T>(((keep >> k) & 1u) ? dzf[k] * d.scale : 0.f);
          store8(dx, v, ov);
        }
      }
    }
  }
  if (WG) {
    float* acc = (float*)ln_lds;
#pragma unroll
    for (int r = 0; r < RPB; ++r) {
      if (wave / WPR == r) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int vi = (i * WPR + wave % WPR) * 64 + lane;
          if (vi < vpr) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int c = vi * 8 + k;
              if (r == 0) {
                acc[c] = ag[i][k];
                acc[H + c] = ab[i][k];
              } else {
                acc[c] += ag[i][k];
                acc[H + c] += ab[i][k];
              }
            }
          }
        }
      }
      __syncthreads();
    }
    float* out = partials + (size_t)blockIdx.x * 2 * H;
    for (int c = threadIdx.x; c < 2 * H; c += kLnThreads) out[c] = acc[c];
  }
}

// 64 columns per block; wave w adds the rows w, w + 4, ... in four
// interleaved chains, then the four waves meet in LDS.  The order is fixed
// by (rows, cols) alone.
__global__ __launch_bounds__(kLnThreads) void ln_fold_k(
    const float* __restrict__ partials, int rows, int cols,
    float* __restrict__ out) {
  __shared__ float red[kLnWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < cols) {
    const float* p = partials + c;
    int r = wave;
    for (; r + 3 * kLnWaves < rows; r += 4 * kLnWaves) {
      a0 += p[(size_t)r * cols];
      a1 += p[(size_t)(r + kLnWaves) * cols];
      a2 += p[(size_t)(r + 2 * kLnWaves) * cols];
      a3 += p[(size_t)(r + 3 * kLnWaves) * cols];
    }
    for (; r < rows; r += kLnWaves) a0 += p[(size_t)r * cols];
  }
  red[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (wave == 0 && c < cols)
    out[c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// one thread per 8-element vector
__global__ __launch_bounds__(kLnThreads) void ln_keep_mask_k(
    unsigned char* __restrict__ out, long long nvec, LnDropout d) {
  const long long v = (long long)blockIdx.x * kLnThreads + threadIdx.x;
  if (v >= nvec) return;
  const unsigned int keep = ln_keep8(d, (unsigned long long)v);
  uint2 w;
  w.x = (keep & 1u) | ((keep >> 1 & 1u) << 8) | ((keep >> 2 & 1u) << 16) |
        ((keep >> 3 & 1u) << 24);
  w.y = (keep >> 4 & 1u) | ((keep >> 5 & 1u) << 8) | ((keep >> 6 & 1u) << 16) |
        ((keep >> 7 & 1u) << 24);
  ((uint2*)out)[v] = w;
}

bool ln_shape_ok(long long M, int H) {
  return M >= 1 && H >= 8 && H <= kLnMaxH && H % 8 == 0;
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

int ln_waves_per_row(int H) { return H <= 1024 ? 1 : (H <= 2048 ? 2 : 4); }

long long ln_groups(long long M, int H) {
  const int rpb = kLnWaves / ln_waves_per_row(H);
  return (M + rpb - 1) / rpb;
}

}  // namespace

hipError_t LnForwardLaunch(const void* x, const void* res, const void* gamma,
                           bool gamma_f32, const void* beta, bool beta_f32,
                           void* y, void* z, float* mean, float* rstd,
                           long long M, int H, int dt, float eps,
                           const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {x, res, gamma, beta, y, z};
  if (!ln_shape_ok(M, H) || !aligned_to(ptrs, 6, 16))
    return hipErrorInvalidValue;
  const int blocks = (int)std::min<long long>(ln_groups(M, H), 2048);
  LN_DISPATCH_T(dt, LN_DISPATCH_H(H, LN_DISPATCH_B(d.t16 > 0, DROP,
      (ln_fwd_k<scalar_t, NV, WPR, DROP><<<blocks, kLnThreads, 0, stream>>>(
          (const scalar_t*)x, (const scalar_t*)res, gamma, gamma_f32, beta,
          beta_f32, (scalar_t*)y, (scalar_t*)z, mean, rstd, M, H, eps, d)))));
  return hipGetLastError();
}

// Every block writes 2H floats of partials next to the 16 rows or more of
// dy, z and dz it moves, so the partial traffic stays a few percent of the
// activation traffic; the cap keeps the fold short.
int LnBackwardBlocks(long long M, int H) {
  const long long want = std::min<long long>((M + 15) / 16, 1024);
  return (int)std::max<long long>(1, std::min(want, ln_groups(M, H)));
}

hipError_t LnBackwardLaunch(const void* dy, const void* z, const float* mean,
                            const float* rstd, const void* gamma,
                            bool gamma_f32, void* dz, void* dx,
                            float* partials, long long M, int H, int dt,
                            const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {dy, z, gamma, dz, dx, partials};
  if (!ln_shape_ok(M, H) || !aligned_to(ptrs, 6, 16) || (d.t16 > 0 && !dx))
    return hipErrorInvalidValue;
  const bool wg = partials != nullptr;
  const int blocks = wg ? LnBackwardBlocks(M, H)
                        : (int)std::min<long long>(ln_groups(M, H), 2048);
  const size_t lds = wg ? (size_t)2 * H * sizeof(float) : 0;
  LN_DISPATCH_T(dt, LN_DISPATCH_H(H, LN_DISPATCH_B(d.t16 > 0, DROP,
      LN_DISPATCH_B(wg, WG,
      (ln_bwd_k<scalar_t, NV, WPR, DROP, WG>
           <<<blocks, kLnThreads, lds, stream>>>(
          (const scalar_t*)dy, (const scalar_t*)z, mean, rstd, gamma,
          gamma_f32, (scalar_t*)dz, (scalar_t*)dx, partials, M, H, d))))));
  return hipGetLastError();
}

hipError_t LnFoldLaunch(const float* partials, int rows, int H, float* out,
                        hipStream_t stream) {
  if (rows < 1 || H < 1) return hipErrorInvalidValue;
  const int cols = 2 * H;
  ln_fold_k<<<(cols + 63) / 64, kLnThreads, 0, stream>>>(partials, rows, cols,
                                                         out);
  return hipGetLastError();
}

hipError_t LnKeepMaskLaunch(unsigned char* out, long long rows, int H,
                            const LnDropout& d, hipStream_t stream) {
  if (rows < 1 || H < 8 || H % 8 != 0 || ((uintptr_t)out % 8) != 0)
    return hipErrorInvalidValue;
  const long long nvec = rows * (H / 8);
  const long long blocks = (nvec + kLnThreads - 1) / kLnThreads;
  if (blocks >= (1LL << 31)) return hipErrorInvalidValue;
  ln_keep_mask_k<<<(unsigned)blocks, kLnThreads, 0, stream>>>(out, nvec, d);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
