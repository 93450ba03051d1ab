// Fused BatchNorm(+Add)+ReLU kernels for CDNA4, NHWC (channels_last).
//
// Motivation (measured, profiles/pipeline_study.md): MIOpen's split
// BN-forward / BN-backward plus the separate ReLU / residual-add elementwise
// passes are ~30% of a ResNet-50 bf16 step's GPU time.  Fusing
// normalize+affine+add+relu into one HBM pass per tensor (and the backward
// reductions into one) removes whole read/write passes.
//
// Layout contract: activations are channels_last-dense [count=N*H*W, C]
// with C contiguous and C % 8 == 0 (every ResNet channel width).  Every
// kernel uses the fixed-channel 8-wide decomposition of bn_common.h: the
// host sizes the grid so (threads * 8) % C == 0, so a thread meets the same
// 8 channels at every grid stride and holds their parameters (two 16-B loads
// per array) and partial sums in registers.  Stats accumulate in fp32 via
// per-block LDS bins (C <= 4096 -> <= 32 KB LDS) flushed with one global
// atomicAdd per channel per block into kBnBanks partial rows (guide G12).
// The rows are zero when a reduction starts: they are the stream's persistent
// workspace, which the kernel that folds them (bn_finalize_k forward,
// bn_bank_reduce_k backward) zeroes again, or per-call memory with a memset.
#include "bn_common.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

// ---- forward stats: per-channel sum and sum-of-squares --------------------
// The read-only stream used to sit at 1.8 TB/s against 7.5 TB/s for the
// apply pass.  Loads in flight were not the limit; the reduction tail was:
//  - narrow C: with C/8 < 64 the lanes of a wave share C/8 octets, so the
//    16 LDS atomicAdds per thread collided up to 64-way (8-way at C = 64);
//    octet_flush folds same-octet lanes by shuffle first
//  - wide C: every block flushes 2C global float atomics, which run at
//    ~1.3 TB/s chip-wide, so 392 blocks at 64x2048x7x7 flushed 6.4 MB to
//    read 12.8 MB; vec8_reduce_grid caps the flushed floats at 2^18
// The smaller grid is made up for by 4 independent loads per thread.
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_k(const T* __restrict__ x,
                                                  long long total, int C,
                                                  float* __restrict__ banks) {
  extern __shared__ float lds[];  // [C] sum, [C] sq
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) lds[c] = 0.f;
  __syncthreads();
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  float rsum[8] = {0}, rsq[8] = {0};
  auto add = [&](const Vec8<T>& v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float f = to_f<T>(v.e[k]);
      rsum[k] += f;
      rsq[k] += f * f;
    }
  };
  long long i = tid;
  for (; i + 3 * nthreads < nvec; i += 4 * nthreads) {
    Vec8<T> v0, v1, v2, v3;
    load8(v0, x, i);
    load8(v1, x, i + nthreads);
    load8(v2, x, i + 2 * nthreads);
    load8(v3, x, i + 3 * nthreads);
    add(v0);
    add(v1);
    add(v2);
    add(v3);
  }
  for (; i < nvec; i += nthreads) {
    Vec8<T> v;
    load8(v, x, i);
    add(v);
  }
  octet_flush(rsum, rsq, c0, C, lds, banks);
}

// ---- forward apply: y = relu(gamma*xhat + beta [+ residual]) --------------
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void bn_apply_relu_k(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    long long total, int C) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  float rm[8], ri[8], rg[8], rb[8];
  load_octet(rm, mean, c0, 0.f);
  load_octet(ri, invstd, c0, 0.f);
  load_octet(rg, gamma, c0, 1.f);
  load_octet(rb, beta, c0, 0.f);
  for (long long i = tid; i < nvec; i += nthreads) {
    Vec8<T> vx, vr, vy;
    load8(vx, x, i);
    if (ADD) load8(vr, res, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float f = bn_preact(to_f<T>(vx.e[k]), rm[k], ri[k], rg[k], rb[k]);
      if (ADD) f += to_f<T>(vr.e[k]);
      vy.e[k] = from_f<T>(f > 0.f ? f : 0.f);
    }
    store8(y, i, vy);
  }
}

// ---- backward stats: g = dy*(y>0); per-channel sum(g), sum(g*xhat);
//      optionally materialize g (residual gradient for the ADD variant)
// FROM_X (no residual only): y is not read; y > 0 is recomputed from x and
// the layer's mean, invstd, gamma and beta (bn_preact, bn_relu_mask).
template <typename T, bool WRITE_G, bool FROM_X>
__global__ __launch_bounds__(256) void bn_bwd_stats_k(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy,
    T* __restrict__ g_out, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, long long total, int C,
    float* __restrict__ banks) {
  extern __shared__ float lds[];  // [C] sum(g), [C] sum(g * xhat)
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) lds[c] = 0.f;
  __syncthreads();
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  // sum(g * xhat) = invstd * sum(g * (x - mean)): invstd is applied once
  // after the loop, which keeps 8 registers out of it
  float rmean[8], racc_g[8] = {0}, racc_gx[8] = {0};
  load_octet(rmean, mean, c0, 0.f);
  float rinv[8], rg[8], rb[8];
  if (FROM_X) {
    load_octet(rinv, invstd, c0, 0.f);
    load_octet(rg, gamma, c0, 1.f);
    load_octet(rb, beta, c0, 0.f);
  }
  // One vector of each of the three tensors in flight per thread.  Two of
  // each took 102-128 VGPRs (4 waves/SIMD against 6-7 here), and holding
  // that form to 7 waves spilled 156-188 B/lane to scratch.
  for (long long i = tid; i < nvec; i += nthreads) {
    Vec8<T> vx, vy, vd, vg;
    load8(vx, x, i);
    if (!FROM_X) load8(vy, y, i);
    load8(vd, dy, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xf = to_f<T>(vx.e[k]);
      const bool on =
          FROM_X ? bn_relu_mask<T>(bn_preact(xf, rmean[k], rinv[k], rg[k], rb[k]))
                 : to_f<T>(vy.e[k]) > 0.f;
      float gv = on ? to_f<T>(vd.e[k]) : 0.f;
      racc_g[k] += gv;
      racc_gx[k] += gv * (xf - rmean[k]);
      if (WRITE_G) vg.e[k] = from_f<T>(gv);
    }
    if (WRITE_G) store8(g_out, i, vg);
  }
  if (!FROM_X) load_octet(rinv, invstd, c0, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) racc_gx[k] *= rinv[k];
  octet_flush(racc_g, racc_gx, c0, C, lds, banks);
}

// reduce the kBnBanks x [2C] partials into sums[2C] (the backward tail).
// CLEAR: the banks are the stream's persistent workspace, and every word
// read is zeroed again for the next reduction.
template <bool CLEAR>
__global__ __launch_bounds__(256) void bn_bank_reduce_k(float* banks,
                                                        float* sums, int C) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < 2 * C;
       c += gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int b = 0; b < kBnBanks; ++b) acc += banks[(size_t)b * 2 * C + c];
    // all loads first: a store in between would order them one by one
    if (CLEAR)
      for (int b = 0; b < kBnBanks; ++b) banks[(size_t)b * 2 * C + c] = 0.f;
    sums[c] = acc;
  }
}

// ---- backward apply: dx = gamma*invstd*(g - sum_g/n - xhat*sum_gx/n) ------
// FROM_G: `dy` is the g = dy*(y>0) that bn_bwd_stats_k<WRITE_G> stored
// (exact: each element is dy itself or 0), so y is not read at all.
// FROM_X (no residual only): y is not read either; y > 0 is recomputed from
// x as in bn_bwd_stats_k<FROM_X>.  That variant keeps gamma in registers for
// the pre-activation and forms gamma * invstd per element (the same rounded
// product) instead of holding a sixth per-channel array.
template <typename T, bool FROM_G, bool FROM_X>
__global__ __launch_bounds__(256) void bn_bwd_apply_k(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy,
    T* __restrict__ dx, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ sum_g,
    const float* __restrict__ sum_gx, long long total, int C,
    float inv_count) {
  static_assert(!(FROM_G && FROM_X), "one source of the ReLU mask");
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  float rmean[8], rinv[8], rgi[8], rsg[8], rsgx[8], rb[8];
  load_octet(rmean, mean, c0, 0.f);
  load_octet(rinv, invstd, c0, 0.f);
  load_octet(rgi, gamma, c0, 1.f);
  load_octet(rsg, sum_g, c0, 0.f);
  load_octet(rsgx, sum_gx, c0, 0.f);
  if (FROM_X) load_octet(rb, beta, c0, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!FROM_X) rgi[k] = rgi[k] * rinv[k];  // FROM_X: rgi stays gamma
    rsg[k] = rsg[k] * inv_count;
    rsgx[k] = rsgx[k] * inv_count;
  }
  for (long long i = tid; i < nvec; i += nthreads) {
    Vec8<T> vx, vy, vd, vo;
    load8(vx, x, i);
    if (!FROM_G && !FROM_X) load8(vy, y, i);
    load8(vd, dy, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xf = to_f<T>(vx.e[k]);
      float gv;
      if (FROM_G) {
        gv = to_f<T>(vd.e[k]);
      } else {
        const bool on =
            FROM_X ? bn_relu_mask<T>(
                         bn_preact(xf, rmean[k], rinv[k], rgi[k], rb[k]))
                   : to_f<T>(vy.e[k]) > 0.f;
        gv = on ? to_f<T>(vd.e[k]) : 0.f;
      }
      float xh = (xf - rmean[k]) * rinv[k];
      const float gi = FROM_X ? rgi[k] * rinv[k] : rgi[k];
      float v = gi * (gv - rsg[k] - xh * rsgx[k]);
      vo.e[k] = from_f<T>(v);
    }
    store8(dx, i, vo);
  }
}

// ---- forward epilogue: fold the banks, mean/invstd, running stats ---------
// One thread per channel over (C + 255) / 256 blocks; the 2 x kBnBanks loads
// of a thread are independent and coalesced across the block.
// CLEAR: the banks are the stream's persistent workspace; the threads
// together read every word of its kBnBanks x [2C] rows, and each zeroes what
// it read for the next reduction.  mean / invstd never alias the banks then.
template <bool CLEAR>
__global__ __launch_bounds__(256) void bn_finalize_k(
    float* __restrict__ banks, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, long long count, float momentum,
    float eps, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float inv_n = 1.0f / (float)count;
  const float ub = count > 1 ? (float)count / (float)(count - 1) : 1.0f;
  float s = 0.f, q = 0.f;
#pragma unroll 16
  for (int b = 0; b < kBnBanks; ++b) {
    s += banks[(size_t)b * 2 * C + c];
    q += banks[(size_t)b * 2 * C + C + c];
  }
  if (CLEAR) {
#pragma unroll 16
    for (int b = 0; b < kBnBanks; ++b) {
      banks[(size_t)b * 2 * C + c] = 0.f;
      banks[(size_t)b * 2 * C + C + c] = 0.f;
    }
  }
  float m = s * inv_n;
  float v = q * inv_n - m * m;
  mean[c] = m;
  invstd[c] = rsqrtf(v + eps);
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * v * ub;
  }
}

// the cl-vec8 kernels read activations and per-channel arrays as 16-B vectors
template <size_t N>
bool aligned16(const void* const (&ptrs)[N]) {
  return aligned_to(ptrs, (int)N, 16);
}

}  // namespace

#define DISPATCH_T(DT, FN)                                        \
  switch (DT) {                                                   \
    case DT_F32: { using scalar_t = float; FN; break; }           \
    case DT_F16: { using scalar_t = __half; FN; break; }          \
    case DT_BF16: { using scalar_t = __hip_bfloat16; FN; break; } \
    default: return hipErrorInvalidValue;                         \
  }

hipError_t BnFinalizeLaunch(float* banks, float* mean, float* invstd,
                            float* running_mean, float* running_var,
                            long long count, float momentum, float eps,
                            int C, bool clear_banks, hipStream_t stream) {
  const int blocks = (C + 255) / 256;
  if (clear_banks)
    bn_finalize_k<true><<<blocks, 256, 0, stream>>>(
        banks, mean, invstd, running_mean, running_var, count, momentum, eps,
        C);
  else
    bn_finalize_k<false><<<blocks, 256, 0, stream>>>(
        banks, mean, invstd, running_mean, running_var, count, momentum, eps,
        C);
  return hipGetLastError();
}

hipError_t BnBankReduceLaunch(float* banks, float* sums, int C,
                              bool clear_banks, hipStream_t stream) {
  const void* const ptrs[] = {sums};
  if (!aligned16(ptrs)) return hipErrorInvalidValue;
  int blocks = (2 * C + 255) / 256;
  if (clear_banks)
    bn_bank_reduce_k<true><<<blocks, 256, 0, stream>>>(banks, sums, C);
  else
    bn_bank_reduce_k<false><<<blocks, 256, 0, stream>>>(banks, sums, C);
  return hipGetLastError();
}

hipError_t BnStatsLaunch(const void* x, long long total, int C, int dt,
                         float* banks, hipStream_t stream) {
  const void* const ptrs[] = {x};
  if (!aligned16(ptrs)) return hipErrorInvalidValue;
  int blocks = vec8_reduce_grid(total, C);
  size_t lds = 2 * (size_t)C * sizeof(float);
  DISPATCH_T(dt, (bn_stats_k<scalar_t><<<blocks, 256, lds, stream>>>(
                     (const scalar_t*)x, total, C, banks)));
  return hipGetLastError();
}

hipError_t BnApplyReluLaunch(const void* x, const void* res, void* y,
                             const float* mean, const float* invstd,
                             const float* gamma, const float* beta,
                             long long total, int C, int dt,
                             hipStream_t stream) {
  const void* const ptrs[] = {x, res, y, mean, invstd, gamma, beta};
  if (!aligned16(ptrs)) return hipErrorInvalidValue;
  int blocks = grid_for(total, C);
  if (res) {
    DISPATCH_T(dt, (bn_apply_relu_k<scalar_t, true><<<blocks, 256, 0, stream>>>(
                       (const scalar_t*)x, (const scalar_t*)res, (scalar_t*)y,
                       mean, invstd, gamma, beta, total, C)));
  } else {
    DISPATCH_T(dt,
               (bn_apply_relu_k<scalar_t, false><<<blocks, 256, 0, stream>>>(
                   (const scalar_t*)x, nullptr, (scalar_t*)y, mean, invstd,
                   gamma, beta, total, C)));
  }
  return hipGetLastError();
}

hipError_t BnBwdStatsLaunch(const void* x, const void* y, const void* dy,
                            void* g_out, const float* mean,
                            const float* invstd, const float* gamma,
                            const float* beta, long long total, int C, int dt,
                            float* banks, hipStream_t stream) {
  const void* const ptrs[] = {x, y, dy, g_out, mean, invstd, gamma, beta};
  if (!aligned16(ptrs)) return hipErrorInvalidValue;
  // the mask comes from y, or without a residual from x, gamma and beta
  if (beta ? (g_out != nullptr || !gamma) : !y) return hipErrorInvalidValue;
  int blocks = vec8_reduce_grid(total, C);
  size_t lds = 2 * (size_t)C * sizeof(float);
  if (beta) {
    DISPATCH_T(
        dt, (bn_bwd_stats_k<scalar_t, false, true><<<blocks, 256, lds, stream>>>(
                (const scalar_t*)x, nullptr, (const scalar_t*)dy, nullptr, mean,
                invstd, gamma, beta, total, C, banks)));
  } else if (g_out) {
    DISPATCH_T(
        dt, (bn_bwd_stats_k<scalar_t, true, false><<<blocks, 256, lds, stream>>>(
                (const scalar_t*)x, (const scalar_t*)y, (const scalar_t*)dy,
                (scalar_t*)g_out, mean, invstd, nullptr, nullptr, total, C,
                banks)));
  } else {
    DISPATCH_T(
        dt,
        (bn_bwd_stats_k<scalar_t, false, false><<<blocks, 256, lds, stream>>>(
            (const scalar_t*)x, (const scalar_t*)y, (const scalar_t*)dy,
            nullptr, mean, invstd, nullptr, nullptr, total, C, banks)));
  }
  return hipGetLastError();
}

hipError_t BnBwdApplyLaunch(const void* x, const void* y, const void* dy,
                            void* dx, const float* mean, const float* invstd,
                            const float* gamma, const float* beta,
                            const float* sum_g, const float* sum_gx,
                            long long total, int C, int dt, float inv_count,
                            hipStream_t stream) {
  const void* const ptrs[] = {x,     y,    dy,    dx,    mean, invstd,
                              gamma, beta, sum_g, sum_gx};
  if (!aligned16(ptrs)) return hipErrorInvalidValue;
  int blocks = grid_for(total, C);
  if (beta) {
    DISPATCH_T(
        dt, (bn_bwd_apply_k<scalar_t, false, true><<<blocks, 256, 0, stream>>>(
                (const scalar_t*)x, nullptr, (const scalar_t*)dy,
                (scalar_t*)dx, mean, invstd, gamma, beta, sum_g, sum_gx, total,
                C, inv_count)));
  } else if (y) {
    DISPATCH_T(
        dt, (bn_bwd_apply_k<scalar_t, false, false><<<blocks, 256, 0, stream>>>(
                (const scalar_t*)x, (const scalar_t*)y, (const scalar_t*)dy,
                (scalar_t*)dx, mean, invstd, gamma, nullptr, sum_g, sum_gx,
                total, C, inv_count)));
  } else {
    DISPATCH_T(
        dt, (bn_bwd_apply_k<scalar_t, true, false><<<blocks, 256, 0, stream>>>(
                (const scalar_t*)x, nullptr, (const scalar_t*)dy,
                (scalar_t*)dx, mean, invstd, gamma, nullptr, sum_g, sum_gx,
                total, C, inv_count)));
  }
  return hipGetLastError();
}

#undef DISPATCH_T

}  // namespace gpu
}  // namespace hvd
