// Fused BatchNorm+ReLU+MaxPool(3, stride 2, padding 1) kernels for CDNA4,
// NHWC: the ResNet stem.  The full-resolution activation y = relu(bn(x)) is
// never stored.  The forward writes the pooled output and, per pooled
// element, the position 0..8 of its arg-max inside the 3x3 window; the
// backward passes rebuild the full-resolution gradient of y on the fly from
// the pooled gradient and those codes (gather form: no atomics, no zero
// fill) and are otherwise the FROM_X passes of bn_kernels.hip.
//
// Layout contract as in bn_kernels.hip: x is channels_last-dense
// [N, H, W, C], C % 8 == 0, C <= 4096, fp32 / fp16 / bf16; the pooled tensors
// are [N, OH, OW, C] with OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1.  A
// thread keeps one channel octet and strides over pixels, so N * H * W must
// stay below 2^31.
#include "bn_common.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

struct PoolGeom {
  int H, W, OH, OW;
};

// first pixel and pixel stride of the calling thread: with (threads * 8) % C
// == 0 the thread's vectors are those of octet `t % (C / 8)` at pixels
// t / (C / 8), + threads / (C / 8), ...
__device__ __forceinline__ void octet_pixels(int C, unsigned& pix,
                                             unsigned& stride) {
  const unsigned vpr = (unsigned)C / 8;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  pix = t / vpr;
  stride = gridDim.x * blockDim.x / vpr;
}

// ---- forward apply + pool --------------------------------------------------
// One thread per pooled channel octet.  Each window element is
// relu(bn_preact(x)) rounded to T, as bn_apply_relu_k<T, false> stores it;
// the max is taken in ATen's scan order (kh outer, kw inner) with ATen's
// update rule, so the first maximum wins.  The rule's NaN term is kept for
// the match with ATen, but nothing reaches it today: f > 0 ? f : 0 stores 0
// for a NaN pre-activation, here as in bn_apply_relu_k.  codes:
// uint8 [N, OH, OW, C], kh * 3 + kw relative to the unclipped window origin
// (2 * oh - 1, 2 * ow - 1).  The 9 x octets of neighbouring windows overlap;
// they are shared through the cache.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_relu_pool_k(
    const T* __restrict__ x, T* __restrict__ pooled,
    unsigned char* __restrict__ codes, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, unsigned npix_out, PoolGeom g, int C) {
  const int c0 = octet_channel(C);
  const unsigned vpr = (unsigned)C / 8;
  const unsigned cv = (unsigned)c0 / 8;
  float rm[8], ri[8], rg[8], rb[8];
  load_octet(rm, mean, c0, 0.f);
  load_octet(ri, invstd, c0, 0.f);
  load_octet(rg, gamma, c0, 1.f);
  load_octet(rb, beta, c0, 0.f);
  unsigned pix, stride;
  octet_pixels(C, pix, stride);
  for (; pix < npix_out; pix += stride) {
    const int ow = (int)(pix % (unsigned)g.OW);
    const unsigned row = pix / (unsigned)g.OW;
    const int oh = (int)(row % (unsigned)g.OH);
    const long long n = row / (unsigned)g.OH;
    float best[8];
    unsigned code[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      best[k] = -INFINITY;
      code[k] = 0;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = 2 * oh - 1 + kh;
      if (h < 0 || h >= g.H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = 2 * ow - 1 + kw;
        if (w < 0 || w >= g.W) continue;
        Vec8<T> vx;
        load8(vx, x, ((n * g.H + h) * g.W + w) * vpr + cv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float f =
              bn_preact(to_f<T>(vx.e[k]), rm[k], ri[k], rg[k], rb[k]);
          const float val = to_f<T>(from_f<T>(f > 0.f ? f : 0.f));
          if (val > best[k] || val != val) {
            best[k] = val;
            code[k] = kh * 3 + kw;
          }
        }
      }
    }
    Vec8<T> vo;
#pragma unroll
    for (int k = 0; k < 8; ++k) vo.e[k] = from_f<T>(best[k]);
    const long long o = (long long)pix * vpr + cv;
    store8(pooled, o, vo);
    uint2 packed;
    packed.x = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
    packed.y = code[4] | code[5] << 8 | code[6] << 16 | code[7] << 24;
    ((uint2*)codes)[o] = packed;
  }
}

// ---- the full-resolution gradient of y over one 2x2 block of input pixels ---
// The backward passes walk the pooled domain: the thread at pooled pixel
// (a, b) owns the input pixels (2a + dh, 2b + dw), dh, dw in {0, 1}, that
// exist.  Those four lie in the windows (a, b), (a, b + 1), (a + 1, b) and
// (a + 1, b + 1) only, so four 16-B loads of gp (eight for fp32) and four 8-B
// loads of the codes serve four pixels, and no lane of a wave takes another
// branch than its neighbours except at the right and bottom borders.
template <typename T>
struct PoolQuad {
  Vec8<T> g[4];    // gp of the four windows; zero where a window does not exist
  uint2 code[4];
};

template <typename T>
__device__ __forceinline__ void pool_quad_load(
    PoolQuad<T>& q, const T* __restrict__ gp,
    const unsigned char* __restrict__ codes, long long o, int a, int b,
    unsigned vpr, const PoolGeom& g) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int da = j >> 1, db = j & 1;
    if (a + da < g.OH && b + db < g.OW) {
      const long long oj = o + ((long long)da * g.OW + db) * vpr;
      load8(q.g[j], gp, oj);
      q.code[j] = ((const uint2*)codes)[oj];
    } else {
      q.g[j].u[0] = make_uint4(0, 0, 0, 0);
      if (sizeof(T) == 4) q.g[j].u[1] = make_uint4(0, 0, 0, 0);
      q.code[j] = make_uint2(0, 0);
    }
  }
}

// d[0..8) for the pixel (2a + dh, 2b + dw): the sum, over the windows that
// cover it, of gp where the window's code names this pixel.  Window j =
// 2 * da + db holds it at kh = dh + 1 - 2 * da, kw = dw + 1 - 2 * db when
// both lie in 0..2.  The sum is fp32, windows in rising (oh, ow) order.
template <typename T>
__device__ __forceinline__ void pool_quad_dy(float (&d)[8],
                                             const PoolQuad<T>& q, int dh,
                                             int dw) {
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int da = j >> 1, db = j & 1;
    const int kh = dh + 1 - 2 * da, kw = dw + 1 - 2 * db;
    if (kh < 0 || kw < 0) continue;  // compile-time after unrolling
    const unsigned me = (unsigned)(kh * 3 + kw);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned word = k < 4 ? q.code[j].x : q.code[j].y;
      const unsigned code = (word >> (8 * (k & 3))) & 0xffu;
      d[k] += code == me ? to_f<T>(q.g[j].e[k]) : 0.f;
    }
  }
}

// ---- backward stats: bn_bwd_stats_k<T, false, FROM_X> with dy gathered -----
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_stats_pool_k(
    const T* __restrict__ x, const T* __restrict__ gp,
    const unsigned char* __restrict__ codes, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, unsigned npix_out, PoolGeom g, int C,
    float* __restrict__ banks) {
  extern __shared__ float lds[];  // [C] sum(g), [C] sum(g * xhat)
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) lds[c] = 0.f;
  __syncthreads();
  const int c0 = octet_channel(C);
  const unsigned vpr = (unsigned)C / 8;
  const unsigned cv = (unsigned)c0 / 8;
  float rmean[8], rinv[8], rg[8], rb[8], racc_g[8] = {0}, racc_gx[8] = {0};
  load_octet(rmean, mean, c0, 0.f);
  load_octet(rinv, invstd, c0, 0.f);
  load_octet(rg, gamma, c0, 1.f);
  load_octet(rb, beta, c0, 0.f);
  unsigned pix, stride;
  octet_pixels(C, pix, stride);
  for (; pix < npix_out; pix += stride) {
    const int b = (int)(pix % (unsigned)g.OW);
    const unsigned row = pix / (unsigned)g.OW;
    const int a = (int)(row % (unsigned)g.OH);
    const long long n = row / (unsigned)g.OH;
    PoolQuad<T> q;
    pool_quad_load(q, gp, codes, (long long)pix * vpr + cv, a, b, vpr, g);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int dh = p >> 1, dw = p & 1;
      const int h = 2 * a + dh, w = 2 * b + dw;
      if (h >= g.H || w >= g.W) continue;
      Vec8<T> vx;
      load8(vx, x, ((n * g.H + h) * g.W + w) * vpr + cv);
      float d[8];
      pool_quad_dy<T>(d, q, dh, dw);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xf = to_f<T>(vx.e[k]);
        const bool on =
            bn_relu_mask<T>(bn_preact(xf, rmean[k], rinv[k], rg[k], rb[k]));
        const float gv = on ? d[k] : 0.f;
        racc_g[k] += gv;
        racc_gx[k] += gv * (xf - rmean[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) racc_gx[k] *= rinv[k];
  octet_flush(racc_g, racc_gx, c0, C, lds, banks);
}

// ---- backward apply: bn_bwd_apply_k<T, false, FROM_X> with dy gathered -----
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_pool_k(
    const T* __restrict__ x, const T* __restrict__ gp,
    const unsigned char* __restrict__ codes, T* __restrict__ dx,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
    unsigned npix_out, PoolGeom g, int C, float inv_count) {
  const int c0 = octet_channel(C);
  const unsigned vpr = (unsigned)C / 8;
  const unsigned cv = (unsigned)c0 / 8;
  float rmean[8], rinv[8], rgi[8], rsg[8], rsgx[8], rb[8];
  load_octet(rmean, mean, c0, 0.f);
  load_octet(rinv, invstd, c0, 0.f);
  load_octet(rgi, gamma, c0, 1.f);
  load_octet(rsg, sum_g, c0, 0.f);
  load_octet(rsgx, sum_gx, c0, 0.f);
  load_octet(rb, beta, c0, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rsg[k] = rsg[k] * inv_count;
    rsgx[k] = rsgx[k] * inv_count;
  }
  unsigned pix, stride;
  octet_pixels(C, pix, stride);
  for (; pix < npix_out; pix += stride) {
    const int b = (int)(pix % (unsigned)g.OW);
    const unsigned row = pix / (unsigned)g.OW;
    const int a = (int)(row % (unsigned)g.OH);
    const long long n = row / (unsigned)g.OH;
    PoolQuad<T> q;
    pool_quad_load(q, gp, codes, (long long)pix * vpr + cv, a, b, vpr, g);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int dh = p >> 1, dw = p & 1;
      const int h = 2 * a + dh, w = 2 * b + dw;
      if (h >= g.H || w >= g.W) continue;
      const long long i = ((n * g.H + h) * g.W + w) * vpr + cv;
      Vec8<T> vx, vo;
      load8(vx, x, i);
      float d[8];
      pool_quad_dy<T>(d, q, dh, dw);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xf = to_f<T>(vx.e[k]);
        const bool on =
            bn_relu_mask<T>(bn_preact(xf, rmean[k], rinv[k], rgi[k], rb[k]));
        float gv = on ? d[k] : 0.f;
        float xh = (xf - rmean[k]) * rinv[k];
        const float gi = rgi[k] * rinv[k];
        float v = gi * (gv - rsg[k] - xh * rsgx[k]);
        vo.e[k] = from_f<T>(v);
      }
      store8(dx, i, vo);
    }
  }
}

template <size_t N>
bool aligned16(const void* const (&ptrs)[N]) {
  return aligned_to(ptrs, (int)N, 16);
}

// H, W >= 1, and every pixel index of x fits the kernels' 32-bit counters
bool pool_geom(long long N, int H, int W, int C, PoolGeom& g) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || C > kBnMaxChannels)
    return false;
  if (N * H * W >= (1LL << 31)) return false;
  g.H = H;
  g.W = W;
  g.OH = (H - 1) / 2 + 1;
  g.OW = (W - 1) / 2 + 1;
  return true;
}

}  // namespace

#define DISPATCH_T(DT, FN)                                        \
  switch (DT) {                                                   \
    case DT_F32: { using scalar_t = float; FN; break; }           \
    case DT_F16: { using scalar_t = __half; FN; break; }          \
    case DT_BF16: { using scalar_t = __hip_bfloat16; FN; break; } \
    default: return hipErrorInvalidValue;                         \
  }

hipError_t BnApplyReluPoolLaunch(const void* x, void* pooled,
                                 unsigned char* codes, const float* mean,
                                 const float* invstd, const float* gamma,
                                 const float* beta, long long N, int H, int W,
                                 int C, int dt, hipStream_t stream) {
  const void* const ptrs[] = {x, pooled, codes, mean, invstd, gamma, beta};
  PoolGeom g;
  if (!aligned16(ptrs) || !pool_geom(N, H, W, C, g))
    return hipErrorInvalidValue;
  const long long npix_out = N * g.OH * g.OW;
  int blocks = grid_for(npix_out * C, C);
  DISPATCH_T(dt, (bn_apply_relu_pool_k<scalar_t><<<blocks, 256, 0, stream>>>(
                     (const scalar_t*)x, (scalar_t*)pooled, codes, mean,
                     invstd, gamma, beta, (unsigned)npix_out, g, C)));
  return hipGetLastError();
}

hipError_t BnBwdStatsPoolLaunch(const void* x, const void* gp,
                                const unsigned char* codes, const float* mean,
                                const float* invstd, const float* gamma,
                                const float* beta, long long N, int H, int W,
                                int C, int dt, float* banks,
                                hipStream_t stream) {
  const void* const ptrs[] = {x, gp, codes, mean, invstd, gamma, beta};
  PoolGeom g;
  if (!aligned16(ptrs) || !pool_geom(N, H, W, C, g))
    return hipErrorInvalidValue;
  // the grid of the dense pass over x: a thread meets as many input pixels
  const long long npix = N * H * W, npix_out = N * g.OH * g.OW;
  int blocks = vec8_reduce_grid(npix * C, C);
  size_t lds = 2 * (size_t)C * sizeof(float);
  DISPATCH_T(dt, (bn_bwd_stats_pool_k<scalar_t><<<blocks, 256, lds, stream>>>(
                     (const scalar_t*)x, (const scalar_t*)gp, codes, mean,
                     invstd, gamma, beta, (unsigned)npix_out, g, C, banks)));
  return hipGetLastError();
}

hipError_t BnBwdApplyPoolLaunch(const void* x, const void* gp,
                                const unsigned char* codes, void* dx,
                                const float* mean, const float* invstd,
                                const float* gamma, const float* beta,
                                const float* sum_g, const float* sum_gx,
                                long long N, int H, int W, int C, int dt,
                                float inv_count, hipStream_t stream) {
  const void* const ptrs[] = {x,     gp,   codes, dx,    mean, invstd,
                              gamma, beta, sum_g, sum_gx};
  PoolGeom g;
  if (!aligned16(ptrs) || !pool_geom(N, H, W, C, g))
    return hipErrorInvalidValue;
  const long long npix_out = N * g.OH * g.OW;
  int blocks = grid_for(npix_out * C, C);
  DISPATCH_T(dt, (bn_bwd_apply_pool_k<scalar_t><<<blocks, 256, 0, stream>>>(
                     (const scalar_t*)x, (const scalar_t*)gp, codes,
                     (scalar_t*)dx, mean, invstd, gamma, beta, sum_g, sum_gx,
                     (unsigned)npix_out, g, C, inv_count)));
  return hipGetLastError();
}

#undef DISPATCH_T

}  // namespace gpu
}  // namespace hvd
