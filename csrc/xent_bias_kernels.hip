// Fused softmax cross-entropy of z = x + bias for the BERT MLM head: logits x
// of [M, V] in fp32 / fp16 / bf16 as the vocabulary GEMM left them, bias fp32
// [V] added in registers.  The forward reads x once, the backward reads it
// once, writes dx once and also returns dbias, the column sums of dx; the
// fp32 sum x + bias and its fp32 gradient are never in memory.
//
// Row access is that of xent_kernels.hip: only the base pointer is 16-B
// aligned, a row starts at any multiple of the element size and is cut into a
// head of up to EPV - 1 elements, 16-B body vectors and a tail (EPV = 16 /
// sizeof(T)).  The cut of row r depends on r * V * sizeof(T) mod 16 alone, so
// the rows r, r + P, r + 2P, ... share one cut, with P = 16 / gcd(16, (V *
// sizeof(T)) mod 16): phase class r mod P.  P is 4 for a bf16 row of 30522,
// at most 8 for a 2-byte type and at most 4 for fp32.
//
// Backward: threads own columns.  A block is given one class p, one column
// tile of 256 body vectors (blockIdx.x) and one chunk of the class's rows
// (blockIdx.y = p * chunks + chunk).  Within a class the body vectors of all
// rows cover the same columns, so a thread keeps one vector position for the
// whole launch: its EPV bias values are loaded once, and EPV fp32 column sums
// of the unrounded dx stay in registers while it walks down the rows, the
// 16-B loads of kXentUnroll rows in flight before the first is used.  Label,
// lse and the incoming gradient of a row are the same for the whole block.
// The head and tail columns of a class, at most EPV - 1 each, go to a column
// tile of their own behind the body tiles, a lane per column with element
// accesses, which keeps them out of the body loop's registers.  At the end a
// thread stores its sums into the block's row of the [P * chunks, V]
// partials: no two threads of a launch share a column and a row chunk, so
// there is no LDS, no shuffle and no barrier, and every block writes every
// column it owns, zeros too.  ColumnFoldLaunch adds the partial rows in a
// fixed order.
//
// Forward: a row reduction as in xent_kernels.hip, a wave per row up to
// kXentWaveMaxV elements and a block beyond, the same (m, s, sum z)
// accumulator and merge rule.  The label is read first and a row with
// ignore_index is not read at all.  The bias under a body vector starts at
// column head_p + i * EPV, which is not 16-B aligned; a small kernel first
// writes P shifted copies shift[p][j] = bias[head_p + j], so the row kernel
// reads EPV / 4 aligned 16-B bias vectors per body vector (at most 1 MB for
// V = 30522, resident in L2).
//
// No atomics anywhere: identical inputs give identical bits.  All arithmetic
// is fp32; dx is rounded once, at the store.
#include <cmath>

#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kXentThreads = 256;
constexpr int kXentWaves = kXentThreads / 64;
constexpr int kXentUnroll = 4;  // 16-B loads of x a lane has in flight

// The helpers down to xent_label_kind are those of xent_kernels.hip, which
// keeps them to its own translation unit.
template <typename T>
union XVec {
  static constexpr int N = 16 / (int)sizeof(T);
  uint4 u;
  T e[16 / sizeof(T)];
  __device__ XVec() {}
};

struct XentCut {
  int head, nvec, tail;
};

// The cut of row `row`, and of every row of its phase class.
template <typename T>
__host__ __device__ __forceinline__ XentCut xent_cut(long long row, int V) {
  constexpr int EPV = 16 / (int)sizeof(T);
  XentCut c;
  const int h = (int)((-(row * V)) & (EPV - 1));
  c.head = h < V ? h : V;
  c.nvec = (V - c.head) / EPV;
  c.tail = V - c.head - c.nvec * EPV;
  return c;
}

struct XentAcc {
  float m, s, sx;
};

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
    e += __expf(v[k] - ms);
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

// 0 the label is ignore_index, 1 it indexes the row, -1 it does neither
__device__ __forceinline__ int xent_label_kind(long long y, long long ignore,
                                               int V) {
  if (y == ignore) return 0;
  return (y >= 0 && y < V) ? 1 : -1;
}

// ---- forward ----------------------------------------------------------------

// shift[p][j] = bias[head_p + j] for the columns of the row, 0 in the padding
template <typename T>
__global__ __launch_bounds__(kXentThreads) void xent_bias_shift_k(
    const float* __restrict__ bias, float* __restrict__ shift, int V, int P,
    int pitch) {
  const long long idx = (long long)blockIdx.x * kXentThreads + threadIdx.x;
  if (idx >= (long long)P * pitch) return;
  const int p = (int)(idx / pitch);
  const int col = xent_cut<T>(p, V).head + (int)(idx - (long long)p * pitch);
  shift[idx] = col < V ? bias[col] : 0.f;
}

// One lane's share of a row of z, lane t of NT.  sh is the row's class's
// shifted bias: sh[i * EPV + k] lies under element k of body vector i.
template <typename T, int NT>
__device__ __forceinline__ XentAcc xent_bias_row_stats(
    const T* __restrict__ xr, const float* __restrict__ bias,
    const float* __restrict__ sh, const XentCut& c, int V, int t) {
  constexpr int EPV = XVec<T>::N;
  constexpr int BV = EPV / 4;  // 16-B bias loads per body vector
  XentAcc a = {-INFINITY, 0.f, 0.f};
  if (t < c.head) {
    const float v[1] = {to_f<T>(xr[t]) + bias[t]};
    xent_add(a, v);
  }
  if (t < c.tail) {
    const int col = V - c.tail + t;
    const float v[1] = {to_f<T>(xr[col]) + bias[col]};
    xent_add(a, v);
  }
  const uint4* __restrict__ body = (const uint4*)(xr + c.head);
  const float4* __restrict__ bbody = (const float4*)sh;
  for (int i = t; i < c.nvec; i += kXentUnroll * NT) {
    XVec<T> v[kXentUnroll];
    float4 b[kXentUnroll][BV];
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j) {
      if (i + j * NT < c.nvec) {
        v[j].u = body[i + j * NT];
#pragma unroll
        for (int q = 0; q < BV; ++q) b[j][q] = bbody[(i + j * NT) * BV + q];
      }
    }
#pragma unroll
    for (int j = 0; j < kXentUnroll; ++j) {
      if (i + j * NT >= c.nvec) break;
      float f[EPV];
#pragma unroll
      for (int q = 0; q < BV; ++q) {
        f[4 * q + 0] = to_f<T>(v[j].e[4 * q + 0]) + b[j][q].x;
        f[4 * q + 1] = to_f<T>(v[j].e[4 * q + 1]) + b[j][q].y;
        f[4 * q + 2] = to_f<T>(v[j].e[4 * q + 2]) + b[j][q].z;
        f[4 * q + 3] = to_f<T>(v[j].e[4 * q + 3]) + b[j][q].w;
      }
      xent_add(a, f);
    }
  }
  return a;
}

// NT = 64: row blockIdx.x * 4 + wave; NT = 256: row blockIdx.x.
template <typename T, int NT>
__global__ __launch_bounds__(kXentThreads) void xent_bias_fwd_k(
    const T* __restrict__ x, const float* __restrict__ bias,
    const float* __restrict__ shift, const long long* __restrict__ labels,
    float* __restrict__ lse, float* __restrict__ row_loss, long long M, int V,
    int P, int pitch, float eps, long long ignore) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long row = NT == 64 ? (long long)blockIdx.x * kXentWaves + wave
                                 : (long long)blockIdx.x;
  if (row >= M) return;  // NT = 64 only, a whole wave at a time
  const long long y = labels[row];
  const int kind = xent_label_kind(y, ignore, V);
  if (kind == 0) {  // the row is not read; all lanes that share it leave
    if ((NT == 64 ? lane : (int)threadIdx.x) == 0) {
      lse[row] = 0.f;
      row_loss[row] = 0.f;
    }
    return;
  }
  const T* __restrict__ xr = x + row * V;
  const XentCut c = xent_cut<T>(row, V);
  const float* __restrict__ sh = shift + (size_t)(row % P) * pitch;
  XentAcc a = xent_bias_row_stats<T, NT>(xr, bias, sh, c, V,
                                         NT == 64 ? lane : (int)threadIdx.x);
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
  float loss = NAN;
  if (kind > 0) {
    loss = fmaf(-(1.0f - eps), to_f<T>(xr[y]) + bias[y], l);
    if (eps > 0.f) loss = fmaf(-(eps / (float)V), a.sx, loss);
  }
  row_loss[row] = loss;
}

// ---- backward ---------------------------------------------------------------

// What the whole block knows of a row: kind as xent_label_kind, the label (-1
// for one that is never an index), lse and the incoming gradient g with its
// two products.  reduction: 0 none (g = dloss[row]), 1 mean (dloss[0] /
// count[0]), 2 sum.  lse and dloss of an ignored row are read and not used.
struct XentBiasRow {
  int kind, y;
  float l, g, gsm, gy;
};

__device__ __forceinline__ XentBiasRow xent_bias_row(
    const long long* __restrict__ labels, const float* __restrict__ lse,
    const float* __restrict__ dloss, const float* __restrict__ count,
    long long row, int V, float eps, long long ignore, int reduction) {
  XentBiasRow w;
  const long long yl = labels[row];
  w.kind = xent_label_kind(yl, ignore, V);
  w.y = (int)yl;
  w.l = lse[row];
  w.g = dloss[reduction == 0 ? row : 0];
  if (reduction == 1) w.g = w.g / count[0];
  if (w.kind < 0) {  // never an index: the whole row, and dbias, say so
    w.g = NAN;
    w.y = -1;
  }
  w.gsm = w.g * (eps / (float)V);
  w.gy = w.g * (1.0f - eps);
  return w;
}

// The gradient of one element z of a row, added to its column's sum
__device__ __forceinline__ float xent_bias_dz(float z, const XentBiasRow& w,
                                              bool at_y, float& acc) {
  float d = fmaf(w.g, __expf(z - w.l), -w.gsm);
  if (at_y) d -= w.gy;
  acc += d;
  return d;
}

// Body tiles: the vector at element offset voff of the NR rows r, r + P, ...
// of the thread's class, all loads first.
template <typename T, int NR>
__device__ __forceinline__ void xent_bias_bwd_body(
    const T* __restrict__ x, const long long* __restrict__ labels,
    const float* __restrict__ lse, const float* __restrict__ dloss,
    const float* __restrict__ count, T* __restrict__ dx, long long r, int P,
    int V, float eps, long long ignore, int reduction, int voff,
    const float (&b)[XVec<T>::N], float (&acc)[XVec<T>::N]) {
  XVec<T> v[NR];
  XentBiasRow w[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long row = r + (long long)j * P;
    w[j] = xent_bias_row(labels, lse, dloss, count, row, V, eps, ignore,
                         reduction);
    // an ignored row is not read
    if (w[j].kind != 0) v[j].u = *(const uint4*)(x + row * V + voff);
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    uint4* __restrict__ o = (uint4*)(dx + (r + (long long)j * P) * V + voff);
    if (w[j].kind == 0) {
      *o = make_uint4(0, 0, 0, 0);
      continue;
    }
#pragma unroll
    for (int k = 0; k < XVec<T>::N; ++k)
      v[j].e[k] = from_f<T>(xent_bias_dz(to_f<T>(v[j].e[k]) + b[k], w[j],
                                         voff + k == w[j].y, acc[k]));
    *o = v[j].u;
  }
}

// The ends tile: column col of the same rows, one element per row.
template <typename T, int NR>
__device__ __forceinline__ void xent_bias_bwd_ends(
    const T* __restrict__ x, const long long* __restrict__ labels,
    const float* __restrict__ lse, const float* __restrict__ dloss,
    const float* __restrict__ count, T* __restrict__ dx, long long r, int P,
    int V, float eps, long long ignore, int reduction, int col, float b,
    float& acc) {
  float v[NR];
  XentBiasRow w[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long row = r + (long long)j * P;
    w[j] = xent_bias_row(labels, lse, dloss, count, row, V, eps, ignore,
                         reduction);
    v[j] = w[j].kind != 0 ? to_f<T>(x[row * V + col]) : 0.f;
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    T* __restrict__ o = dx + (r + (long long)j * P) * V + col;
    if (w[j].kind == 0)
      *o = from_f<T>(0.f);
    else
      *o = from_f<T>(xent_bias_dz(v[j] + b, w[j], col == w[j].y, acc));
  }
}

// grid (column tiles + 1, P * chunks).  The chunks of a class are
// ceil(ceil(M / P) / chunks) rows of it each, the last ones shorter or empty.
// Column tile blockIdx.x < gridDim.x - 1 holds 256 body vectors, a lane each.
// The last one is the ends tile: its lanes 0 .. EPV - 1 take the head columns
// of the class and lanes EPV .. 2 EPV - 1 the tail columns, with twice the
// rows in flight, since an element load is all a row costs them.
template <typename T>
__global__ __launch_bounds__(kXentThreads) void xent_bias_bwd_k(
    const T* __restrict__ x, const float* __restrict__ bias,
    const long long* __restrict__ labels, const float* __restrict__ lse,
    const float* __restrict__ dloss, const float* __restrict__ count,
    T* __restrict__ dx, float* __restrict__ partials, long long M, int V,
    int P, int chunks, float eps, long long ignore, int reduction) {
  constexpr int EPV = XVec<T>::N;
  const int t = threadIdx.x;
  const int p = blockIdx.y / chunks;
  const int chunk = blockIdx.y - p * chunks;
  const XentCut c = xent_cut<T>(p, V);
  // rows p + P * k of the class, k in [k0, k1)
  const long long n = p < M ? (M - p + P - 1) / P : 0;
  const long long rpc = ((M + P - 1) / P + chunks - 1) / chunks;
  const long long k0 = min(n, (long long)chunk * rpc);
  const long long k1 = min(n, k0 + rpc);
  float* __restrict__ prow = partials + (size_t)blockIdx.y * V;
  long long k = k0;

  if (blockIdx.x == gridDim.x - 1) {
    int col = -1;
    if (t < c.head) col = t;
    if (t >= EPV && t - EPV < c.tail) col = V - c.tail + (t - EPV);
    if (col < 0) return;
    const float b = bias[col];
    float acc = 0.f;
    for (; k + 2 * kXentUnroll <= k1; k += 2 * kXentUnroll)
      xent_bias_bwd_ends<T, 2 * kXentUnroll>(x, labels, lse, dloss, count, dx,
                                             p + k * P, P, V, eps, ignore,
                                             reduction, col, b, acc);
    for (; k < k1; ++k)
      xent_bias_bwd_ends<T, 1>(x, labels, lse, dloss, count, dx, p + k * P, P,
                               V, eps, ignore, reduction, col, b, acc);
    prow[col] = acc;
    return;
  }

  const long long i = (long long)blockIdx.x * kXentThreads + t;
  if (i >= c.nvec) return;
  const int voff = c.head + (int)i * EPV;
  float b[EPV], acc[EPV];
#pragma unroll
  for (int q = 0; q < EPV; ++q) {
    b[q] = bias[voff + q];
    acc[q] = 0.f;
  }
  for (; k + kXentUnroll <= k1; k += kXentUnroll)
    xent_bias_bwd_body<T, kXentUnroll>(x, labels, lse, dloss, count, dx,
                                       p + k * P, P, V, eps, ignore, reduction,
                                       voff, b, acc);
  for (; k < k1; ++k)
    xent_bias_bwd_body<T, 1>(x, labels, lse, dloss, count, dx, p + k * P, P,
                             V, eps, ignore, reduction, voff, b, acc);
#pragma unroll
  for (int q = 0; q < EPV; ++q) prow[voff + q] = acc[q];
}

bool xent_bias_shape_ok(long long M, long long V) {
  return M >= 1 && V >= 1 && V <= kXentMaxV && M <= kXentMaxM;
}

long long xent_bias_tiles(int V, int dt) {
  const long long epv = dt == DT_F32 ? 4 : 8;
  return std::max<long long>(1, (V / epv + kXentThreads - 1) / kXentThreads);
}

#define XENT_BIAS_DISPATCH_T(DT, ...)                                   \
  switch (DT) {                                                         \
    case DT_F32: { using scalar_t = float; __VA_ARGS__; break; }        \
    case DT_F16: { using scalar_t = __half; __VA_ARGS__; break; }       \
    case DT_BF16: { using scalar_t = __hip_bfloat16; __VA_ARGS__; break; } \
    default: return hipErrorInvalidValue;                               \
  }

}  // namespace

int XentBiasPhases(int V, int dt) {
  const long long rem = ((long long)V * (dt == DT_F32 ? 4 : 2)) % 16;
  return rem == 0 ? 1 : (int)(16 / std::__gcd(16LL, rem));
}

// Row chunks of each phase class, by the rule of GeluRowChunks: a chunk costs
// one partial row, V floats written here and read by the fold, so it has at
// least 16 rows of its class, and there are no more chunks than bring the grid
// of body tiles x P x chunks blocks to about kBlocks = 1024, 4 per CU.
int XentBiasRowChunks(long long M, int V, int dt) {
  constexpr long long kMinRows = 16, kBlocks = 1024;
  const long long P = XentBiasPhases(V, dt);
  const long long class_rows = (M + P - 1) / P;
  const long long by_rows = (class_rows + kMinRows - 1) / kMinRows;
  const long long by_grid =
      std::max<long long>(1, kBlocks / (xent_bias_tiles(V, dt) * P));
  return (int)std::max<long long>(1, std::min(by_rows, by_grid));
}

hipError_t XentBiasForwardLaunch(const void* x, const float* bias,
                                 const long long* labels, float* shift,
                                 float* lse, float* row_loss, long long M,
                                 int V, int dt, float eps,
                                 long long ignore_index, hipStream_t stream) {
  if (!xent_bias_shape_ok(M, V) || !x || !bias || !labels || !shift || !lse ||
      !row_loss || ((uintptr_t)x % 16) != 0 || ((uintptr_t)shift % 16) != 0 ||
      !(eps >= 0.f && eps < 1.f))
    return hipErrorInvalidValue;
  const int P = XentBiasPhases(V, dt);
  const int pitch = (int)XentBiasPitch(V);
  const unsigned sgrid =
      (unsigned)(((long long)P * pitch + kXentThreads - 1) / kXentThreads);
  XENT_BIAS_DISPATCH_T(dt, (xent_bias_shift_k<scalar_t>
                                <<<sgrid, kXentThreads, 0, stream>>>(
      bias, shift, V, P, pitch)));
  if (V <= kXentWaveMaxV) {
    const unsigned grid = (unsigned)((M + kXentWaves - 1) / kXentWaves);
    XENT_BIAS_DISPATCH_T(dt, (xent_bias_fwd_k<scalar_t, 64>
                                  <<<grid, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, bias, shift, labels, lse, row_loss, M, V, P, pitch,
        eps, ignore_index)));
  } else {
    XENT_BIAS_DISPATCH_T(dt, (xent_bias_fwd_k<scalar_t, kXentThreads>
                                  <<<(unsigned)M, kXentThreads, 0, stream>>>(
        (const scalar_t*)x, bias, shift, labels, lse, row_loss, M, V, P, pitch,
        eps, ignore_index)));
  }
  return hipGetLastError();
}

hipError_t XentBiasBackwardLaunch(const void* x, const float* bias,
                                  const long long* labels, const float* lse,
                                  const float* dloss, const float* count,
                                  void* dx, float* partials, long long M,
                                  int V, int dt, float eps,
                                  long long ignore_index, int reduction,
                                  hipStream_t stream) {
  if (!xent_bias_shape_ok(M, V) || !x || !bias || !labels || !lse || !dloss ||
      !dx || !partials || ((uintptr_t)x % 16) != 0 ||
      ((uintptr_t)dx % 16) != 0 || !(eps >= 0.f && eps < 1.f) ||
      reduction < 0 || reduction > 2 || (reduction == 1 && !count))
    return hipErrorInvalidValue;
  const int P = XentBiasPhases(V, dt);
  const int chunks = XentBiasRowChunks(M, V, dt);
  const dim3 grid((unsigned)xent_bias_tiles(V, dt) + 1,  // + the ends tile
                  (unsigned)(P * chunks));
  XENT_BIAS_DISPATCH_T(dt, (xent_bias_bwd_k<scalar_t>
                                <<<grid, kXentThreads, 0, stream>>>(
      (const scalar_t*)x, bias, labels, lse, dloss, count, (scalar_t*)dx,
      partials, M, V, P, chunks, eps, ignore_index, reduction)));
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
