// Fused softmax cross-entropy over rows of V contiguous logits, [M, V], for
// the BERT MLM loss: one read of the logits in the forward, one read and one
// write in the backward, no softmax and no fp32 copy ever in memory.
//
// Row access.  V is whatever the vocabulary is (30522 = 2 * 15261), so a row
// starts at any multiple of the element size: only the base pointer is 16-B
// aligned.  Every row is therefore cut, from its own start address, into
//   head  the 0 .. 16 / sizeof(T) - 1 elements up to the next 16-B boundary,
//         one lane each;
//   body  16-B vectors, lane t of the NT lanes that share the row taking
//         vectors t, t + NT, ...; kXentUnroll loads are issued before the
//         first of them is used;
//   tail  what is left after the last whole vector, one lane each.
// No thread owns a column: the phase of the cut changes from row to row (with
// period 4 for a bf16 row of 30522, up to 8 for an odd V).
//
// Work split.  Rows of up to kXentWaveMaxV elements get one wave each, four
// rows per 256-thread block, and meet neither LDS nor a barrier; longer rows
// get a block each (NT = 256), whose four waves combine through LDS.  The
// backward is elementwise once the row's scalars are known, so at small M a
// long row is also cut into column chunks across gridDim.y.
//
// Forward.  A lane keeps a running maximum m, the sum s of exp(x - m) and the
// plain sum of x (label smoothing needs it), updated once per vector: the
// vector's own maximum first, then one rescale of s and EPV exponentials.
// Lanes merge by (m, s) + (m', s') = (M, s exp(m - M) + s' exp(m' - M)), M =
// max(m, m'), through xor shuffles, then the waves of a block in rising wave
// order.  The merge is commutative bit for bit, so every lane of a wave ends
// with the same value, and nothing depends on timing: no atomics anywhere,
// identical inputs give identical bits.
//
// All arithmetic is fp32; dx is rounded once, at the store.
#include <cmath>

#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kXentThreads = 256;
constexpr int kXentWaves = kXentThreads / 64;
// 16-B loads a lane has in flight; 8 measured no faster at [8192, 30522] and
// slower at [1024, 30522] (docs/benchmarks.md)
constexpr int kXentUnroll = 4;

template <typename T>
union XVec {
  static constexpr int N = 16 / (int)sizeof(T);
  uint4 u;
  T e[16 / sizeof(T)];
  __device__ XVec() {}
};

// The cut of row `row`: x + row * V is 16-B aligned after `head` elements.
struct XentCut {
  int head, nvec, tail;
};

template <typename T>
__device__ __forceinline__ XentCut xent_cut(long long row, int V) {
  constexpr int EPV = XVec<T>::N;
  XentCut c;
  c.head = min((int)((-(row * V)) & (EPV - 1)), V);
  c.nvec = (V - c.head) / EPV;
  c.tail = V - c.head - c.nvec * EPV;
  return c;
}

struct XentAcc {
  float m, s, sx;
};

// exp(a - b) for the running sums; b = -inf (nothing finite seen yet) counts
// as 0, so that exp(-inf - -inf) is never formed
__device__ __forceinline__ float xent_safe(float m) {
  return m == -INFINITY ? 0.f : m;
}

template <int N>
__device__ __forceinline__ void xent_add(XentAcc& a, const float (&v)[N]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < N; ++k) mx = fmaxf(mx, v[k]);
  const float mn = fmaxf(a.m, mx);
  const float ms = xent_safe(mn);
  float e = 0.f, sx = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    e += __expf(v[k] - ms);  // a NaN logit is dropped by fmaxf and lands here
    sx += v[k];
  }
  a.s = fmaf(a.s, __expf(a.m - ms), e);
  a.sx += sx;
  a.m = mn;
}

__device__ __forceinline__ void xent_merge(XentAcc& a, float m, float s,
                                           float sx) {
  const float mn = fmaxf(a.m, m);
  const float ms = xent_safe(mn);
  a.s = a.s * __expf(a.m - ms) + s * __expf(m - ms);
  a.sx += sx;
  a.m = mn;
}

__device__ __forceinline__ void xent_wave_reduce(XentAcc& a) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
    xent_merge(a, __shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64),
               __shfl_xor(a.sx, o, 64));
}

// One lane's share of a row, lane t of NT.
template <typename T, int NT>
__device__ __forceinline__ XentAcc xent_row_stats(const T* __restrict__ xr,
                                                  const XentCut& c, int V,
                                                  int t) {
  constexpr int EPV = XVec<T>::N;
  XentAcc a = {-INFINITY, 0.f, 0.f};
  if (t < c.head) {
    const float v[1] = {to_f<T>(xr[t])};
    xent_add(a, v);
  }
  if (t < c.tail) {
    const float v[1] = {to_f<T>(xr[V - c.tail + t])};
    xent_add(a, v);
  }
  const uint4* __restrict__ body = (const uint4*)(xr + c.head);
  // kXentUnroll loads are issued before the first is used, in the last pass
  // too, where the ones past the row are masked out
  for (int i = t; i < c.nvec; i += kXentUnroll * NT) {
    XVec<T> v[kXentUnroll];
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j)
      if (i + j * NT < c.nvec) v[j].u = body[i + j * NT];
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j) {
      if (i + j * NT >= c.nvec) break;
      float f[EPV];
#pragma unroll
      for (int k = 0; k < EPV; ++k) f[k] = to_f<T>(v[j].e[k]);
      xent_add(a, f);
    }
  }
  return a;
}

// 0 the label is ignore_index, 1 it indexes the row, -1 it does neither
__device__ __forceinline__ int xent_label_kind(long long y, long long ignore,
                                               int V) {
  if (y == ignore) return 0;
  return (y >= 0 && y < V) ? 1 : -1;
}

// NT = 64: row blockIdx.x * 4 + wave; NT = 256: row blockIdx.x.
template <typename T, int NT>
__global__ __launch_bounds__(kXentThreads) void xent_fwd_k(
    const T* __restrict__ x, const long long* __restrict__ labels,
    float* __restrict__ lse, float* __restrict__ row_loss, long long M, int V,
    float eps, long long ignore) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long row = NT == 64 ? (long long)blockIdx.x * kXentWaves + wave
                                 : (long long)blockIdx.x;
  if (row >= M) return;  // NT = 64 only, a whole wave at a time
  const T* __restrict__ xr = x + row * V;
  const XentCut c = xent_cut<T>(row, V);
  XentAcc a = xent_row_stats<T, NT>(xr, c, V, NT == 64 ? lane : threadIdx.x);
  xent_wave_reduce(a);
  if (NT != 64) {
    __shared__ float red[kXentWaves][3];
    if (lane == 0) {
      red[wave][0] = a.m;
      red[wave][1] = a.s;
      red[wave][2] = a.sx;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    a.m = red[0][0];
    a.s = red[0][1];
    a.sx = red[0][2];
#pragma unroll
    for (int w = 1; w < kXentWaves; ++w)
      xent_merge(a, red[w][0], red[w][1], red[w][2]);
  } else if (lane != 0) {
    return;
  }
  const float l = a.m + logf(a.s);
  lse[row] = l;
  const long long y = labels[row];
  const int kind = xent_label_kind(y, ignore, V);
  float loss = 0.f;
  if (kind < 0) {
    loss = NAN;
  } else if (kind > 0) {
    loss = fmaf(-(1.0f - eps), to_f<T>(xr[y]), l);
    if (eps > 0.f) loss = fmaf(-(eps / (float)V), a.sx, loss);
  }
  row_loss[row] = loss;
}

// One block: out[0] = the sum of the M row losses (over the count of labels
// that are not ignore_index with `mean`), out[1] = that count.  Thread t adds
// rows t, t + 256, ... in rising order, then the 256 partial sums meet in a
// fixed tree.
__global__ __launch_bounds__(kXentThreads) void xent_fold_k(
    const float* __restrict__ row_loss, const long long* __restrict__ labels,
    long long M, long long ignore, bool mean, float* __restrict__ out) {
  __shared__ float ssum[kXentThreads];
  __shared__ float scnt[kXentThreads];
  float s = 0.f;
  long long n = 0;
  long long r = threadIdx.x;
  for (; r + 7 * kXentThreads < M; r += 8 * kXentThreads) {
    float v[8];
    long long y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = row_loss[r + j * kXentThreads];
      y[j] = labels[r + j * kXentThreads];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s += v[j];
      n += y[j] != ignore;
    }
  }
  for (; r < M; r += kXentThreads) {
    s += row_loss[r];
    n += labels[r] != ignore;
  }
  ssum[threadIdx.x] = s;
  scnt[threadIdx.x] = (float)n;
  __syncthreads();
  for (int o = kXentThreads / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      ssum[threadIdx.x] += ssum[threadIdx.x + o];
      scnt[threadIdx.x] += scnt[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = mean ? ssum[0] / scnt[0] : ssum[0];
    out[1] = scnt[0];
  }
}

// dx of the EPV elements of one vector whose first column is c0
template <typename T>
__device__ __forceinline__ void xent_dx_vec(XVec<T>& v, int c0, int y,
                                            float l, float g, float gsm,
                                            float gy) {
#pragma unroll
  for (int k = 0; k < XVec<T>::N; ++k) {
    float d = fmaf(g, __expf(to_f<T>(v.e[k]) - l), -gsm);
    if (c0 + k == y) d -= gy;
    v.e[k] = from_f<T>(d);
  }
}

// NT = 64: row blockIdx.x * 4 + wave, the whole row.  NT = 256: row
// blockIdx.x, body vectors [blockIdx.y * per, (blockIdx.y + 1) * per) with
// per = ceil(ceil(V / EPV) / gridDim.y); chunk 0 also takes head and tail.
// reduction: 0 none (g = dloss[row]), 1 mean (dloss[0] / count[0]), 2 sum.
template <typename T, int NT>
__global__ __launch_bounds__(kXentThreads) void xent_bwd_k(
    const T* __restrict__ x, const long long* __restrict__ labels,
    const float* __restrict__ lse, const float* __restrict__ dloss,
    const float* __restrict__ count, T* __restrict__ dx, long long M, int V,
    float eps, long long ignore, int reduction) {
  constexpr int EPV = XVec<T>::N;
  const int t = NT == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const long long row =
      NT == 64 ? (long long)blockIdx.x * kXentWaves + (threadIdx.x >> 6)
               : (long long)blockIdx.x;
  if (row >= M) return;
  const XentCut c = xent_cut<T>(row, V);
  int v0 = 0, v1 = c.nvec;
  bool ends = true;
  if (NT != 64) {
    const int per = ((V + EPV - 1) / EPV + gridDim.y - 1) / gridDim.y;
    v0 = min(c.nvec, (int)blockIdx.y * per);
    v1 = min(c.nvec, v0 + per);
    ends = blockIdx.y == 0;
  }
  const T* __restrict__ xr = x + row * V;
  T* __restrict__ dr = dx + row * V;
  uint4* __restrict__ dbody = (uint4*)(dr + c.head);
  const long long yl = labels[row];
  const int kind = xent_label_kind(yl, ignore, V);

  if (kind == 0) {
    // the zeros are written, and the logits are not read
    if (ends && t < c.head) dr[t] = from_f<T>(0.f);
    if (ends && t < c.tail) dr[V - c.tail + t] = from_f<T>(0.f);
    for (int i = v0 + t; i < v1; i += NT) dbody[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  float g = dloss[reduction == 0 ? row : 0];
  if (reduction == 1) g = g / count[0];
  int y = (int)yl;
  if (kind < 0) {  // never an index: the whole row says so
    g = NAN;
    y = -1;
  }
  const float l = lse[row];
  const float gsm = g * (eps / (float)V);
  const float gy = g * (1.0f - eps);

  if (ends && t < c.head) {
    float d = fmaf(g, __expf(to_f<T>(xr[t]) - l), -gsm);
    if (t == y) d -= gy;
    dr[t] = from_f<T>(d);
  }
  if (ends && t < c.tail) {
    const int col = V - c.tail + t;
    float d = fmaf(g, __expf(to_f<T>(xr[col]) - l), -gsm);
    if (col == y) d -= gy;
    dr[col] = from_f<T>(d);
  }
  const uint4* __restrict__ body = (const uint4*)(xr + c.head);
  for (int i = v0 + t; i < v1; i += kXentUnroll * NT) {
    XVec<T> v[kXentUnroll];
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j)
      if (i + j * NT < v1) v[j].u = body[i + j * NT];
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j) {
      if (i + j * NT >= v1) break;
      xent_dx_vec<T>(v[j], c.head + (i + j * NT) * EPV, y, l, g, gsm, gy);
      dbody[i + j * NT] = v[j].u;
    }
  }
}

bool xent_shape_ok(long long M, long long V) {
  return M >= 1 && V >= 1 && V <= kXentMaxV && M <= kXentMaxM;
}

#define XENT_DISPATCH_T(DT, ...)                                        \
  switch (DT) {                                                         \
    case DT_F32: { using scalar_t = float; __VA_ARGS__; break; }        \
    case DT_F16: { using scalar_t = __half; __VA_ARGS__; break; }       \
    case DT_BF16: { using scalar_t = __hip_bfloat16; __VA_ARGS__; break; } \
    default: return hipErrorInvalidValue;                               \
  }

}  // namespace

// Column chunks of a block-per-row backward.  A chunk is never shorter than
// one unrolled pass of the block (256 lanes x kXentUnroll vectors), and there
// are no more chunks than bring the grid to about kBlocks = 1024 blocks, 4
// per CU.  Rows of the wave-per-row path are never cut.
int XentBackwardChunks(long long M, int V, int dt) {
  constexpr long long kBlocks = 1024;
  if (V <= kXentWaveMaxV) return 1;
  const long long epv = dt == DT_F32 ? 4 : 8;
  const long long pass = kXentThreads * kXentUnroll * epv;
  const long long by_len = std::max<long long>(1, V / pass);
  const long long by_grid = std::max<long long>(1, kBlocks / M);
  return (int)std::min(by_len, by_grid);
}

hipError_t XentForwardLaunch(const void* x, const long long* labels,
                             float* lse, float* row_loss, long long M, int V,
                             int dt, float eps, long long ignore_index,
                             hipStream_t stream) {
  if (!xent_shape_ok(M, V) || !x || !labels || !lse || !row_loss ||
      ((uintptr_t)x % 16) != 0 || !(eps >= 0.f && eps < 1.f))
    return hipErrorInvalidValue;
  if (V <= kXentWaveMaxV) {
    const unsigned grid = (unsigned)((M + kXentWaves - 1) / kXentWaves);
    XENT_DISPATCH_T(dt, (xent_fwd_k<scalar_t, 64>
                             <<<grid, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, labels, lse, row_loss, M, V, eps, ignore_index)));
  } else {
    XENT_DISPATCH_T(dt, (xent_fwd_k<scalar_t, kXentThreads>
                             <<<(unsigned)M, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, labels, lse, row_loss, M, V, eps, ignore_index)));
  }
  return hipGetLastError();
}

hipError_t XentFoldLaunch(const float* row_loss, const long long* labels,
                          long long M, long long ignore_index, bool mean,
                          float* out, hipStream_t stream) {
  if (M < 1 || !row_loss || !labels || !out) return hipErrorInvalidValue;
  xent_fold_k<<<1, kXentThreads, 0, stream>>>(row_loss, labels, M,
                                              ignore_index, mean, out);
  return hipGetLastError();
}

hipError_t XentBackwardLaunch(const void* x, const long long* labels,
                              const float* lse, const float* dloss,
                              const float* count, void* dx, long long M, int V,
                              int dt, float eps, long long ignore_index,
                              int reduction, hipStream_t stream) {
  if (!xent_shape_ok(M, V) || !x || !labels || !lse || !dloss || !dx ||
      ((uintptr_t)x % 16) != 0 || ((uintptr_t)dx % 16) != 0 ||
      !(eps >= 0.f && eps < 1.f) || reduction < 0 || reduction > 2 ||
      (reduction == 1 && !count))
    return hipErrorInvalidValue;
  if (V <= kXentWaveMaxV) {
    const unsigned grid = (unsigned)((M + kXentWaves - 1) / kXentWaves);
    XENT_DISPATCH_T(dt, (xent_bwd_k<scalar_t, 64>
                             <<<grid, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, labels, lse, dloss, count, (scalar_t*)dx, M, V,
        eps, ignore_index, reduction)));
  } else {
    const dim3 grid((unsigned)M, (unsigned)XentBackwardChunks(M, V, dt));
    XENT_DISPATCH_T(dt, (xent_bwd_k<scalar_t, kXentThreads>
                             <<<grid, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, labels, lse, dloss, count, (scalar_t*)dx, M, V,
        eps, ignore_index, reduction)));
  }
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
