// SyncBatchNorm kernels for CDNA4: everything around the two stats
// allreduces (horovod_amd/torch/sync_batch_norm.py) in at most two HBM
// passes per direction, with every statistic carried in fp32.
//
// Layout contract: activations are a dense (outer, C, inner) block.
//   planar        (N, C, L) contiguous: outer = N, inner = L  (NCHW, NCDHW,
//                 (N,C,L))
//   channels-last rows of C contiguous channels: outer = N*L, inner = 1
//                 (channels_last 4-D/5-D, and (N,C))
// Three decompositions, each used by all four big passes:
//   planar   block (c, s) walks split s of channel c's outer*inner elements
//            in vectors of 16 / 8 / sizeof(T) bytes, whichever the run
//            length and the base pointers allow (2-byte dtypes with odd L
//            take the scalar instantiation); per-channel parameters are
//            block-uniform
//   cl-vec8  inner == 1, C % 8 == 0, C <= 4096: the fixed-channel 8-wide
//            decomposition of bn_kernels.hip (shared pieces: bn_common.h),
//            with a wave-level fold in front of the LDS bins
//   cl-tile  inner == 1, any C: 64 channels x 4 rows per block, scalar
// Reductions go wave shuffle -> LDS -> one atomicAdd per (block, channel);
// the element count travels as the last word of the forward stats buffer
// and is only ever read back on the device.
#include "bn_common.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

template <int VB> struct RawVec;
template <> struct RawVec<16> { using type = uint4; };
template <> struct RawVec<8> { using type = uint2; };
template <> struct RawVec<4> { using type = unsigned int; };
template <> struct RawVec<2> { using type = unsigned short; };

template <typename T, int VB>
union PVec {
  typename RawVec<VB>::type r;
  T e[VB / sizeof(T)];
  __device__ PVec() {}
};

template <typename T, int VB>
__device__ __forceinline__ void pload(PVec<T, VB>& v, const T* p) {
  v.r = *(const typename RawVec<VB>::type*)p;
}
template <typename T, int VB>
__device__ __forceinline__ void pstore(T* p, const PVec<T, VB>& v) {
  *(typename RawVec<VB>::type*)p = v.r;
}

// Block (c, s) of a planar (N, C, L) tensor: visit the element offset of
// every W-wide vector of channel c that belongs to split s of S.  Vector j
// of the channel (j < N * L/W) sits in sample j / (L/W); consecutive
// threads take consecutive vectors and the S blocks of a channel
// interleave, so a wave reads one contiguous span.  (n, l) advance
// incrementally: one division per thread, none per vector.
template <int W, typename F>
__device__ __forceinline__ void planar_walk(unsigned N, unsigned C, unsigned L,
                                            unsigned S, unsigned c, unsigned s,
                                            F&& f) {
  const unsigned Lv = L / W;
  const unsigned nv = N * Lv;  // host guarantees N * L < 2^31
  const unsigned stride = S * 256;
  const unsigned dn = stride / Lv, dl = stride % Lv;
  unsigned j = s * 256 + threadIdx.x;
  unsigned n = j / Lv, l = j % Lv;
  for (; j < nv; j += stride) {
    f(((size_t)n * C + c) * L + (size_t)l * W);
    n += dn;
    l += dl;
    if (l >= Lv) {
      l -= Lv;
      ++n;
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Block-wide sum of two values; the result is valid in thread 0.
__device__ __forceinline__ void block_sum2(float& a, float& b) {
  __shared__ float red[2][4];
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// cl-tile reduction tail: acc of thread (row lane rl, channel lane cl) ->
// one atomicAdd per channel of the block.
__device__ __forceinline__ void tile_flush2(float a, float b, long long c,
                                            int C, float* out0, float* out1) {
  __shared__ float red[2][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  red[0][rl][cl] = a;
  red[1][rl][cl] = b;
  __syncthreads();
  if (rl == 0 && c < C) {
    atomicAdd(&out0[c],
              red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl]);
    atomicAdd(&out1[c],
              red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl]);
  }
}

// ---- forward stats ---------------------------------------------------------
// out = [sum(C), sqsum(C), count], zeroed by the launcher.
template <typename T, int VB>
__global__ __launch_bounds__(256) void sbn_stats_planar_k(
    const T* __restrict__ x, unsigned N, unsigned C, unsigned L, unsigned S,
    float count, float* __restrict__ out) {
  constexpr int W = VB / sizeof(T);
  const unsigned c = blockIdx.x / S, s = blockIdx.x % S;
  float a = 0.f, q = 0.f;
  planar_walk<W>(N, C, L, S, c, s, [&](size_t off) {
    PVec<T, VB> v;
    pload(v, x + off);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float f = to_f<T>(v.e[k]);
      a += f;
      q += f * f;
    }
  });
  block_sum2(a, q);
  if (threadIdx.x == 0) {
    atomicAdd(&out[c], a);
    atomicAdd(&out[C + c], q);
    if (blockIdx.x == 0) out[2 * (size_t)C] = count;
  }
}

// banked like bn_stats_k: kBnBanks rows of [2C] partials
template <typename T>
__global__ __launch_bounds__(256) void sbn_stats_vec8_k(
    const T* __restrict__ x, long long total, int C,
    float* __restrict__ banks) {
  extern __shared__ float lds[];  // [C] sum, [C] sqsum
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
  // 4 independent loads in flight per thread: wide-C grids are small (see
  // vec8_reduce_grid), so the memory parallelism has to come from here
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

template <typename T>
__global__ __launch_bounds__(256) void sbn_stats_tile_k(
    const T* __restrict__ x, long long rows, int C, int S, float count,
    float* __restrict__ out) {
  const long long c = (long long)(blockIdx.x / S) * 64 + (threadIdx.x & 63);
  const long long r0 = (long long)(blockIdx.x % S) * 4 + (threadIdx.x >> 6);
  float a = 0.f, q = 0.f;
  if (c < C) {
    for (long long r = r0; r < rows; r += (long long)S * 4) {
      float f = to_f<T>(x[r * C + c]);
      a += f;
      q += f * f;
    }
  }
  tile_flush2(a, q, c, C, out, out + C);
  if (blockIdx.x == 0 && threadIdx.x == 0) out[2 * (size_t)C] = count;
}

// Fold kBnBanks x [2C] partials (the cl-vec8 reductions) into out[0..2C);
// has_count appends the element count as out[2C].
__global__ __launch_bounds__(256) void sbn_fold_banks_k(
    const float* __restrict__ banks, int C, float count, bool has_count,
    float* __restrict__ out) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < 2 * C;
       c += gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int b = 0; b < kBnBanks; ++b) acc += banks[(size_t)b * 2 * C + c];
    out[c] = acc;
  }
  if (has_count && blockIdx.x == 0 && threadIdx.x == 0) out[2 * C] = count;
}

// ---- finalize: reduced [sum, sqsum, count] -> mean, invstd, running stats --
__global__ __launch_bounds__(256) void sbn_finalize_k(
    const float* __restrict__ stats, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, float momentum, float eps, int C) {
  const float n = stats[2 * (size_t)C];
  const float inv_n = 1.0f / n;
  const float ub = n / fmaxf(n - 1.0f, 1.0f);
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C;
       c += gridDim.x * blockDim.x) {
    float m = stats[c] * inv_n;
    float v = fmaxf(stats[C + c] * inv_n - m * m, 0.f);
    mean[c] = m;
    invstd[c] = rsqrtf(v + eps);
    if (running_mean)
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    if (running_var)
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * v * ub;
  }
}

// ---- forward apply: y = (x - mean) * invstd * w + b ------------------------
template <typename T, int VB>
__global__ __launch_bounds__(256) void sbn_apply_planar_k(
    const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ w,
    const float* __restrict__ b, unsigned N, unsigned C, unsigned L,
    unsigned S) {
  constexpr int W = VB / sizeof(T);
  const unsigned c = blockIdx.x / S, s = blockIdx.x % S;
  const float m = mean[c];
  const float sc = invstd[c] * (w ? w[c] : 1.f);
  const float sh = b ? b[c] : 0.f;
  planar_walk<W>(N, C, L, S, c, s, [&](size_t off) {
    PVec<T, VB> v, o;
    pload(v, x + off);
#pragma unroll
    for (int k = 0; k < W; ++k)
      o.e[k] = from_f<T>((to_f<T>(v.e[k]) - m) * sc + sh);
    pstore(y + off, o);
  });
}

template <typename T>
__global__ __launch_bounds__(256) void sbn_apply_vec8_k(
    const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ w,
    const float* __restrict__ b, long long total, int C) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  // fixed-channel decomposition (see bn_stats_k)
  const int c0 = octet_channel(C);
  float rm[8], rs[8], rw[8], rb[8];
  load_octet(rm, mean, c0, 0.f);
  load_octet(rs, invstd, c0, 0.f);
  load_octet(rw, w, c0, 1.f);
  load_octet(rb, b, c0, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) rs[k] *= rw[k];
  for (long long i = tid; i < nvec; i += nthreads) {
    Vec8<T> vx, vy;
    load8(vx, x, i);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      vy.e[k] = from_f<T>((to_f<T>(vx.e[k]) - rm[k]) * rs[k] + rb[k]);
    store8(y, i, vy);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sbn_apply_tile_k(
    const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ w,
    const float* __restrict__ b, long long rows, int C, int S) {
  const long long c = (long long)(blockIdx.x / S) * 64 + (threadIdx.x & 63);
  const long long r0 = (long long)(blockIdx.x % S) * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float m = mean[c];
  const float sc = invstd[c] * (w ? w[c] : 1.f);
  const float sh = b ? b[c] : 0.f;
  for (long long r = r0; r < rows; r += (long long)S * 4)
    y[r * C + c] = from_f<T>((to_f<T>(x[r * C + c]) - m) * sc + sh);
}

// ---- backward reduce: sums = [sum(dy)(C), sum(dy * xhat)(C)] ---------------
template <typename T, int VB>
__global__ __launch_bounds__(256) void sbn_bwd_reduce_planar_k(
    const T* __restrict__ x, const T* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    unsigned N, unsigned C, unsigned L, unsigned S, float* __restrict__ out) {
  constexpr int W = VB / sizeof(T);
  const unsigned c = blockIdx.x / S, s = blockIdx.x % S;
  const float m = mean[c], is = invstd[c];
  float a = 0.f, q = 0.f;
  planar_walk<W>(N, C, L, S, c, s, [&](size_t off) {
    PVec<T, VB> vx, vd;
    pload(vx, x + off);
    pload(vd, dy + off);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float g = to_f<T>(vd.e[k]);
      a += g;
      q += g * ((to_f<T>(vx.e[k]) - m) * is);
    }
  });
  block_sum2(a, q);
  if (threadIdx.x == 0) {
    atomicAdd(&out[c], a);
    atomicAdd(&out[C + c], q);
  }
}

// banked like bn_bwd_stats_k: kBnBanks rows of [2C] partials
template <typename T>
__global__ __launch_bounds__(256) void sbn_bwd_reduce_vec8_k(
    const T* __restrict__ x, const T* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    long long total, int C, float* __restrict__ banks) {
  extern __shared__ float lds[];  // [C] sum(dy), [C] sum(dy * xhat)
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) lds[c] = 0.f;
  __syncthreads();
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  float rmean[8], rinv[8], racc_g[8] = {0}, racc_gx[8] = {0};
  load_octet(rmean, mean, c0, 0.f);
  load_octet(rinv, invstd, c0, 0.f);
  auto add = [&](const Vec8<T>& vx, const Vec8<T>& vd) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float g = to_f<T>(vd.e[k]);
      racc_g[k] += g;
      racc_gx[k] += g * ((to_f<T>(vx.e[k]) - rmean[k]) * rinv[k]);
    }
  };
  // 2 x 2 independent loads in flight per thread (see sbn_stats_vec8_k)
  long long i = tid;
  for (; i + nthreads < nvec; i += 2 * nthreads) {
    Vec8<T> vx0, vd0, vx1, vd1;
    load8(vx0, x, i);
    load8(vd0, dy, i);
    load8(vx1, x, i + nthreads);
    load8(vd1, dy, i + nthreads);
    add(vx0, vd0);
    add(vx1, vd1);
  }
  for (; i < nvec; i += nthreads) {
    Vec8<T> vx, vd;
    load8(vx, x, i);
    load8(vd, dy, i);
    add(vx, vd);
  }
  octet_flush(racc_g, racc_gx, c0, C, lds, banks);
}

template <typename T>
__global__ __launch_bounds__(256) void sbn_bwd_reduce_tile_k(
    const T* __restrict__ x, const T* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    long long rows, int C, int S, float* __restrict__ out) {
  const long long c = (long long)(blockIdx.x / S) * 64 + (threadIdx.x & 63);
  const long long r0 = (long long)(blockIdx.x % S) * 4 + (threadIdx.x >> 6);
  float a = 0.f, q = 0.f;
  if (c < C) {
    const float m = mean[c], is = invstd[c];
    for (long long r = r0; r < rows; r += (long long)S * 4) {
      float g = to_f<T>(dy[r * C + c]);
      a += g;
      q += g * ((to_f<T>(x[r * C + c]) - m) * is);
    }
  }
  tile_flush2(a, q, c, C, out, out + C);
}

// ---- backward apply: dx = w*invstd*(dy - sum_dy/n - xhat*sum_dy_xhat/n) ----
// sums are the allreduced ones; n is the allreduced count, read on device.
template <typename T, int VB>
__global__ __launch_bounds__(256) void sbn_bwd_apply_planar_k(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ w, const float* __restrict__ sums,
    const float* __restrict__ count, unsigned N, unsigned C, unsigned L,
    unsigned S) {
  constexpr int W = VB / sizeof(T);
  const unsigned c = blockIdx.x / S, s = blockIdx.x % S;
  const float inv_n = 1.0f / count[0];
  const float m = mean[c], is = invstd[c];
  const float gi = is * (w ? w[c] : 1.f);
  const float k1 = sums[c] * inv_n, k2 = sums[C + c] * inv_n;
  planar_walk<W>(N, C, L, S, c, s, [&](size_t off) {
    PVec<T, VB> vx, vd, vo;
    pload(vx, x + off);
    pload(vd, dy + off);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float xh = (to_f<T>(vx.e[k]) - m) * is;
      vo.e[k] = from_f<T>(gi * (to_f<T>(vd.e[k]) - k1 - xh * k2));
    }
    pstore(dx + off, vo);
  });
}

template <typename T>
__global__ __launch_bounds__(256) void sbn_bwd_apply_vec8_k(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ w, const float* __restrict__ sums,
    const float* __restrict__ count, long long total, int C) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const long long nvec = total / 8;
  const int c0 = octet_channel(C);
  const float inv_n = 1.0f / count[0];
  float rmean[8], rinv[8], rgi[8], rk1[8], rk2[8];
  load_octet(rmean, mean, c0, 0.f);
  load_octet(rinv, invstd, c0, 0.f);
  load_octet(rgi, w, c0, 1.f);
  load_octet(rk1, sums, c0, 0.f);
  load_octet(rk2, sums + C, c0, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rgi[k] *= rinv[k];
    rk1[k] *= inv_n;
    rk2[k] *= inv_n;
  }
  for (long long i = tid; i < nvec; i += nthreads) {
    Vec8<T> vx, vd, vo;
    load8(vx, x, i);
    load8(vd, dy, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float xh = (to_f<T>(vx.e[k]) - rmean[k]) * rinv[k];
      vo.e[k] = from_f<T>(rgi[k] * (to_f<T>(vd.e[k]) - rk1[k] - xh * rk2[k]));
    }
    store8(dx, i, vo);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sbn_bwd_apply_tile_k(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ w, const float* __restrict__ sums,
    const float* __restrict__ count, long long rows, int C, int S) {
  const long long c = (long long)(blockIdx.x / S) * 64 + (threadIdx.x & 63);
  const long long r0 = (long long)(blockIdx.x % S) * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float inv_n = 1.0f / count[0];
  const float m = mean[c], is = invstd[c];
  const float gi = is * (w ? w[c] : 1.f);
  const float k1 = sums[c] * inv_n, k2 = sums[C + c] * inv_n;
  for (long long r = r0; r < rows; r += (long long)S * 4) {
    float xh = (to_f<T>(x[r * C + c]) - m) * is;
    dx[r * C + c] = from_f<T>(gi * (to_f<T>(dy[r * C + c]) - k1 - xh * k2));
  }
}

// ---- host-side shape logic -------------------------------------------------
enum Path { kPlanar, kVec8, kTile };

struct Plan {
  Path path;
  long long outer, C, inner;  // after folding the degenerate layouts
  int vb;                     // planar vector bytes
  unsigned S;                 // planar / tile: splits per channel (group)
  int blocks;
};

bool vec8_shape(long long C, long long inner) {
  return inner == 1 && C > 1 && C % 8 == 0 && C <= 4096;
}

// per_thread: vectors (planar) or rows (tile) each thread should cover
// before a block flushes; 1 for the elementwise passes.
// ptrs: the activation tensors; params: the fp32 per-channel arrays, which
// only the cl-vec8 kernels read as vectors.
bool make_plan(long long outer, long long C, long long inner, size_t esize,
               const void* const* ptrs, int nptrs, const void* const* params,
               int nparams, int per_thread, Plan* p) {
  if (outer <= 0 || C <= 0 || inner <= 0) return false;
  // a single channel is one planar run whatever the nominal layout
  if (C == 1) {
    inner *= outer;
    outer = 1;
  }
  p->outer = outer;
  p->C = C;
  p->inner = inner;
  p->vb = 0;
  p->S = 1;
  if (vec8_shape(C, inner) && aligned_to(ptrs, nptrs, 16) &&
      aligned_to(params, nparams, 16)) {
    p->path = kVec8;
    p->blocks = per_thread > 1 ? vec8_reduce_grid(outer * C, (int)C)
                               : grid_for(outer * C, (int)C);
    return true;
  }
  if (C >= (1LL << 31)) return false;
  if (inner == 1) {
    p->path = kTile;
    long long groups = (C + 63) / 64;
    long long want = (outer + 4LL * per_thread - 1) / (4LL * per_thread);
    long long cap = std::max<long long>(1, 2048 / groups);
    p->S = (unsigned)std::min(std::max<long long>(want, 1), cap);
    long long blocks = groups * p->S;
    if (blocks >= (1LL << 31)) return false;
    p->blocks = (int)blocks;
    return true;
  }
  if (outer * inner >= (1LL << 31)) return false;
  p->path = kPlanar;
  size_t run_bytes = (size_t)inner * esize;
  if (run_bytes % 16 == 0 && aligned_to(ptrs, nptrs, 16)) {
    p->vb = 16;
  } else if (run_bytes % 8 == 0 && aligned_to(ptrs, nptrs, 8)) {
    p->vb = 8;
  } else {
    p->vb = (int)esize;
  }
  long long nv = outer * (inner / (p->vb / (long long)esize));
  long long want = (nv + 256LL * per_thread - 1) / (256LL * per_thread);
  long long cap = std::max<long long>(1, 2048 / C);
  p->S = (unsigned)std::min(std::max<long long>(want, 1), cap);
  long long blocks = C * p->S;
  if (blocks >= (1LL << 31)) return false;
  p->blocks = (int)blocks;
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

// planar kernels come in three vector widths: 16 B, 8 B and scalar
#define DISPATCH_VB(VBYTES, FN)                                      \
  if ((VBYTES) == 16) { constexpr int kVB = 16; FN; }                \
  else if ((VBYTES) == 8) { constexpr int kVB = 8; FN; }             \
  else { constexpr int kVB = (int)sizeof(scalar_t); FN; }

static size_t dt_size(int dt) { return dt == DT_F32 ? 4 : 2; }

bool SyncBnBanked(long long C, long long inner) { return vec8_shape(C, inner); }

hipError_t SyncBnStatsLaunch(const void* x, long long outer, long long C,
                             long long inner, int dt, float* banks, float* out,
                             hipStream_t stream) {
  if (dt != DT_F32 && dt != DT_F16 && dt != DT_BF16)
    return hipErrorInvalidValue;
  const void* ptrs[] = {x};
  Plan p;
  if (!make_plan(outer, C, inner, dt_size(dt), ptrs, 1, nullptr, 0, 8, &p))
    return hipErrorInvalidValue;
  const float count = (float)(outer * inner);
  if (p.path == kVec8) {
    if (!banks) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(
        banks, 0, (size_t)kBnBanks * 2 * C * sizeof(float), stream);
    if (e != hipSuccess) return e;
    size_t lds = 2 * (size_t)C * sizeof(float);
    DISPATCH_T(dt, (sbn_stats_vec8_k<scalar_t><<<p.blocks, 256, lds, stream>>>(
                       (const scalar_t*)x, outer * C, (int)C, banks)));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    sbn_fold_banks_k<<<(int)((2 * C + 255) / 256), 256, 0, stream>>>(
        banks, (int)C, count, true, out);
    return hipGetLastError();
  }
  hipError_t e =
      hipMemsetAsync(out, 0, (size_t)(2 * C + 1) * sizeof(float), stream);
  if (e != hipSuccess) return e;
  if (p.path == kTile) {
    DISPATCH_T(dt, (sbn_stats_tile_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                       (const scalar_t*)x, p.outer, (int)C, (int)p.S, count,
                       out)));
  } else {
    DISPATCH_T(dt, DISPATCH_VB(p.vb, (sbn_stats_planar_k<scalar_t, kVB>
                                      <<<p.blocks, 256, 0, stream>>>(
                                          (const scalar_t*)x,
                                          (unsigned)p.outer, (unsigned)C,
                                          (unsigned)p.inner, p.S, count,
                                          out))));
  }
  return hipGetLastError();
}

hipError_t SyncBnFinalizeLaunch(const float* stats, float* mean, float* invstd,
                                float* running_mean, float* running_var,
                                float momentum, float eps, int C,
                                hipStream_t stream) {
  int blocks = std::min((C + 255) / 256, 2048);
  sbn_finalize_k<<<blocks, 256, 0, stream>>>(stats, mean, invstd, running_mean,
                                            running_var, momentum, eps, C);
  return hipGetLastError();
}

hipError_t SyncBnApplyLaunch(const void* x, void* y, const float* mean,
                             const float* invstd, const float* w,
                             const float* b, long long outer, long long C,
                             long long inner, int dt, hipStream_t stream) {
  const void* ptrs[] = {x, y};
  const void* params[] = {mean, invstd, w, b};
  Plan p;
  if (!make_plan(outer, C, inner, dt_size(dt), ptrs, 2, params, 4, 1, &p))
    return hipErrorInvalidValue;
  if (p.path == kVec8) {
    DISPATCH_T(dt, (sbn_apply_vec8_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                       (const scalar_t*)x, (scalar_t*)y, mean, invstd, w, b,
                       outer * C, (int)C)));
  } else if (p.path == kTile) {
    DISPATCH_T(dt, (sbn_apply_tile_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                       (const scalar_t*)x, (scalar_t*)y, mean, invstd, w, b,
                       p.outer, (int)C, (int)p.S)));
  } else {
    DISPATCH_T(dt, DISPATCH_VB(p.vb, (sbn_apply_planar_k<scalar_t, kVB>
                                      <<<p.blocks, 256, 0, stream>>>(
                                          (const scalar_t*)x, (scalar_t*)y,
                                          mean, invstd, w, b,
                                          (unsigned)p.outer, (unsigned)C,
                                          (unsigned)p.inner, p.S))));
  }
  return hipGetLastError();
}

hipError_t SyncBnBwdReduceLaunch(const void* x, const void* dy,
                                 const float* mean, const float* invstd,
                                 long long outer, long long C, long long inner,
                                 int dt, float* banks, float* out,
                                 hipStream_t stream) {
  const void* ptrs[] = {x, dy};
  const void* params[] = {mean, invstd};
  Plan p;
  if (!make_plan(outer, C, inner, dt_size(dt), ptrs, 2, params, 2, 8, &p))
    return hipErrorInvalidValue;
  if (p.path == kVec8) {
    if (!banks) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(
        banks, 0, (size_t)kBnBanks * 2 * C * sizeof(float), stream);
    if (e != hipSuccess) return e;
    size_t lds = 2 * (size_t)C * sizeof(float);
    DISPATCH_T(dt,
               (sbn_bwd_reduce_vec8_k<scalar_t><<<p.blocks, 256, lds, stream>>>(
                   (const scalar_t*)x, (const scalar_t*)dy, mean, invstd,
                   outer * C, (int)C, banks)));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    sbn_fold_banks_k<<<(int)((2 * C + 255) / 256), 256, 0, stream>>>(
        banks, (int)C, 0.f, false, out);
    return hipGetLastError();
  }
  hipError_t e =
      hipMemsetAsync(out, 0, (size_t)(2 * C) * sizeof(float), stream);
  if (e != hipSuccess) return e;
  if (p.path == kTile) {
    DISPATCH_T(dt,
               (sbn_bwd_reduce_tile_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                   (const scalar_t*)x, (const scalar_t*)dy, mean, invstd,
                   p.outer, (int)C, (int)p.S, out)));
  } else {
    DISPATCH_T(dt, DISPATCH_VB(p.vb, (sbn_bwd_reduce_planar_k<scalar_t, kVB>
                                      <<<p.blocks, 256, 0, stream>>>(
                                          (const scalar_t*)x,
                                          (const scalar_t*)dy, mean, invstd,
                                          (unsigned)p.outer, (unsigned)C,
                                          (unsigned)p.inner, p.S, out))));
  }
  return hipGetLastError();
}

hipError_t SyncBnBwdApplyLaunch(const void* x, const void* dy, void* dx,
                                const float* mean, const float* invstd,
                                const float* w, const float* sums,
                                const float* count, long long outer,
                                long long C, long long inner, int dt,
                                hipStream_t stream) {
  const void* ptrs[] = {x, dy, dx};
  const void* params[] = {mean, invstd, w, sums};
  Plan p;
  if (!make_plan(outer, C, inner, dt_size(dt), ptrs, 3, params, 4, 1, &p))
    return hipErrorInvalidValue;
  if (p.path == kVec8) {
    DISPATCH_T(dt,
               (sbn_bwd_apply_vec8_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                   (const scalar_t*)x, (const scalar_t*)dy, (scalar_t*)dx, mean,
                   invstd, w, sums, count, outer * C, (int)C)));
  } else if (p.path == kTile) {
    DISPATCH_T(dt,
               (sbn_bwd_apply_tile_k<scalar_t><<<p.blocks, 256, 0, stream>>>(
                   (const scalar_t*)x, (const scalar_t*)dy, (scalar_t*)dx, mean,
                   invstd, w, sums, count, p.outer, (int)C, (int)p.S)));
  } else {
    DISPATCH_T(dt, DISPATCH_VB(p.vb, (sbn_bwd_apply_planar_k<scalar_t, kVB>
                                      <<<p.blocks, 256, 0, stream>>>(
                                          (const scalar_t*)x,
                                          (const scalar_t*)dy, (scalar_t*)dx,
                                          mean, invstd, w, sums, count,
                                          (unsigned)p.outer, (unsigned)C,
                                          (unsigned)p.inner, p.S))));
  }
  return hipGetLastError();
}

#undef DISPATCH_VB
#undef DISPATCH_T

}  // namespace gpu
}  // namespace hvd
