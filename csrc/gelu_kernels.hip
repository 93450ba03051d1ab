// Fused bias + GELU + dropout for the BERT feed-forward:
// out = dropout(gelu(u + bias), p) over u of [M, N], and its backward
// du = dy * keep * scale * gelu'(u + bias), dbias = column sums of du.
//
// A thread owns one column octet (8 adjacent columns) for the whole launch:
// its 8 bias values sit in registers, and it walks down rows with 16-B
// accesses (two per vector for fp32).  A wave covers 512 adjacent columns of a
// row, the four waves of a block take the rows r, r + 1, r + 2, r + 3 (mod 4)
// of one column tile, and the grid is column tiles x row chunks.  Each thread
// issues the loads of several rows before it touches the first of them, as
// many rows as make eight 16-B loads per lane in flight (forward: 8 rows of a
// 2-byte type, 4 of fp32; backward, which reads dy and u: 4 and 2).  Lanes
// past N / 8 in the last column tile idle.
//
// The backward keeps 8 fp32 column sums of the unrounded du per thread when
// the bias gradient is wanted.  The waves of a block meet through LDS in
// rising wave order and write the block's 512-column segment of partial row
// blockIdx.y of [chunks, N]; the partial rows are folded by ln_fold_k
// (ColumnFoldLaunch).  No atomics anywhere: identical inputs give identical
// bits.
//
// The dropout mask is ln_keep8 (ln_philox.h) of vector row * (N / 8) + octet,
// recomputed in forward and backward and never stored.  All arithmetic is
// fp32 with one rounding to T at the store.
#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kGeluThreads = 256;
constexpr int kGeluWaves = kGeluThreads / 64;
constexpr int kGeluTile = 512;  // columns of a wave

// rows a thread has in flight: 16-B loads per row = tensors * sizeof(T) / 2
template <typename T, int TENSORS>
constexpr int gelu_unroll() { return 16 / (TENSORS * (int)sizeof(T)); }

constexpr float kSqrtHalf = 0.70710678118654752f;      // 1 / sqrt(2)
constexpr float kInvSqrt2Pi = 0.39894228040143268f;    // 1 / sqrt(2 pi)
constexpr float kTanhK = 0.79788456080286536f;         // sqrt(2 / pi)
constexpr float kTanhC = 0.044715f;

// 1 / (1 + exp(-x)) with the hardware's exp2 and reciprocal (about 1 ulp
// each); exp(-x) = inf gives 0, exp(-x) = 0 gives 1
__device__ __forceinline__ float gelu_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}

// Phi(v) = 0.5 (1 + erf(v / sqrt 2)) given e = exp(-v^2 / 2), which the
// derivative needs anyway.  erfc(x) = t (a1 + t (a2 + ... t a5)) exp(-x^2),
// t = 1 / (1 + p x), x >= 0: Abramowitz and Stegun 7.1.26, |error| <=
// 1.5e-7, a few fmas where the library erff is the larger half of the
// kernel's arithmetic (these kernels are close to compute-bound).  Taking
// 0.5 erfc(|x|) for v < 0 also avoids the cancellation of 1 + erf there.
__device__ __forceinline__ float gelu_cdf(float v, float e) {
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * kSqrtHalf, fabsf(v),
                                             1.0f));
  float q = fmaf(t, 1.061405429f, -1.453152027f);
  q = fmaf(t, q, 1.421413741f);
  q = fmaf(t, q, -0.284496736f);
  q = fmaf(t, q, 0.254829592f);
  const float h = 0.5f * t * q * e;
  return v < 0.f ? h : 1.0f - h;
}

// exact form: v Phi(v); tanh form: 0.5 v (1 + tanh(z)) = v * sigmoid(2 z),
// z = k (v + c v^3)
template <bool TANH>
__device__ __forceinline__ float gelu_f(float v) {
  if (TANH) {
    const float z2 = 2.0f * kTanhK * v * fmaf(kTanhC * v, v, 1.0f);
    return v * gelu_sigmoid(z2);
  }
  return v * gelu_cdf(v, __expf(-0.5f * v * v));
}

// exact: Phi(v) + v phi(v); tanh: s + v s (1 - s) * d(2 z)/dv with
// s = sigmoid(2 z)
template <bool TANH>
__device__ __forceinline__ float gelu_df(float v) {
  if (TANH) {
    const float vv = v * v;
    const float z2 = 2.0f * kTanhK * v * fmaf(kTanhC, vv, 1.0f);
    const float s = gelu_sigmoid(z2);
    const float dz2 = 2.0f * kTanhK * fmaf(3.0f * kTanhC, vv, 1.0f);
    return fmaf(v * s * (1.0f - s), dz2, s);
  }
  const float e = __expf(-0.5f * v * v);
  return fmaf(v * kInvSqrt2Pi, e, gelu_cdf(v, e));
}

// the 8 bias values of the octet at column c0: fp32 or T; null reads as 0
template <typename T>
__device__ __forceinline__ void gelu_bias8(float (&r)[8], const void* bias,
                                           bool f32, int c0) {
  if (!bias || f32 || sizeof(T) == 4) {
    load_octet(r, (const float*)bias, c0, 0.f);
  } else {
    Vec8<T> v;
    load8(v, (const T*)bias, c0 / 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = to_f<T>(v.e[k]);
  }
}

// The rows [r0, r1) of chunk blockIdx.y; the chunks are ceil(M / gridDim.y)
// rows each, the last ones shorter or empty.
__device__ __forceinline__ void gelu_chunk(long long M, long long& r0,
                                           long long& r1) {
  const long long rpc = (M + gridDim.y - 1) / gridDim.y;
  r0 = min(M, (long long)blockIdx.y * rpc);
  r1 = min(M, r0 + rpc);
}

// NR rows row, row + kGeluWaves, ... of the thread's octet: all loads first
template <typename T, bool TANH, bool DROP, int NR>
__device__ __forceinline__ void gelu_fwd_rows(
    const T* __restrict__ u, T* __restrict__ out, const float (&b)[8],
    long long row, int vpr, int oct, const LnDropout& d) {
  Vec8<T> uv[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j)
    load8(uv[j], u, (row + j * kGeluWaves) * vpr + oct);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long v = (row + j * kGeluWaves) * vpr + oct;
    unsigned int keep = 0xFFu;
    if (DROP) keep = ln_keep8(d, (unsigned long long)v);
    Vec8<T> ov;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float g = gelu_f<TANH>(to_f<T>(uv[j].e[k]) + b[k]);
      if (DROP) g = ((keep >> k) & 1u) ? g * d.scale : 0.f;
      ov.e[k] = from_f<T>(g);
    }
    store8(out, v, ov);
  }
}

template <typename T, bool TANH, bool DROP>
__global__ __launch_bounds__(kGeluThreads) void gelu_fwd_k(
    const T* __restrict__ u, const void* __restrict__ bias, bool bias_f32,
    T* __restrict__ out, long long M, int N, LnDropout d) {
  constexpr int UNR = gelu_unroll<T, 1>();
  const int wave = threadIdx.x >> 6;
  const int vpr = N / 8;
  const int oct = blockIdx.x * (kGeluTile / 8) + (threadIdx.x & 63);
  if (oct >= vpr) return;
  float b[8];
  gelu_bias8<T>(b, bias, bias_f32, oct * 8);
  long long r0, r1;
  gelu_chunk(M, r0, r1);
  long long row = r0 + wave;
  for (; row + (UNR - 1) * kGeluWaves < r1; row += UNR * kGeluWaves)
    gelu_fwd_rows<T, TANH, DROP, UNR>(u, out, b, row, vpr, oct, d);
  for (; row < r1; row += kGeluWaves)
    gelu_fwd_rows<T, TANH, DROP, 1>(u, out, b, row, vpr, oct, d);
}

// BG: acc[k] += the unrounded du of column k of the octet
template <typename T, bool TANH, bool DROP, bool BG, int NR>
__device__ __forceinline__ void gelu_bwd_rows(
    const T* __restrict__ dy, const T* __restrict__ u, T* __restrict__ du,
    const float (&b)[8], float (&acc)[8], long long row, int vpr, int oct,
    const LnDropout& d) {
  Vec8<T> gv[NR], uv[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long v = (row + j * kGeluWaves) * vpr + oct;
    load8(gv[j], dy, v);
    load8(uv[j], u, v);
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long v = (row + j * kGeluWaves) * vpr + oct;
    unsigned int keep = 0xFFu;
    if (DROP) keep = ln_keep8(d, (unsigned long long)v);
    Vec8<T> ov;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float g = to_f<T>(gv[j].e[k]);
      if (DROP) g = ((keep >> k) & 1u) ? g * d.scale : 0.f;
      g *= gelu_df<TANH>(to_f<T>(uv[j].e[k]) + b[k]);
      if (BG) acc[k] += g;
      ov.e[k] = from_f<T>(g);
    }
    store8(du, v, ov);
  }
}

template <typename T, bool TANH, bool DROP, bool BG>
__global__ __launch_bounds__(kGeluThreads) void gelu_bwd_k(
    const T* __restrict__ dy, const T* __restrict__ u,
    const void* __restrict__ bias, bool bias_f32, T* __restrict__ du,
    float* __restrict__ partials, long long M, int N, LnDropout d) {
  // the sums of waves 1 .. 3, [wave - 1][k][lane]: conflict-free both ways
  __shared__ float red[BG ? (kGeluWaves - 1) * 8 * 64 : 1];
  constexpr int UNR = gelu_unroll<T, 2>();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int vpr = N / 8;
  const int oct = blockIdx.x * (kGeluTile / 8) + lane;
  const bool live = oct < vpr;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (live) {
    float b[8];
    gelu_bias8<T>(b, bias, bias_f32, oct * 8);
    long long r0, r1;
    gelu_chunk(M, r0, r1);
    long long row = r0 + wave;
    for (; row + (UNR - 1) * kGeluWaves < r1; row += UNR * kGeluWaves)
      gelu_bwd_rows<T, TANH, DROP, BG, UNR>(dy, u, du, b, acc, row, vpr, oct,
                                            d);
    for (; row < r1; row += kGeluWaves)
      gelu_bwd_rows<T, TANH, DROP, BG, 1>(dy, u, du, b, acc, row, vpr, oct,
                                          d);
  }
  if (BG) {
    if (wave > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[((wave - 1) * 8 + k) * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
      for (int w = 1; w < kGeluWaves; ++w)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += red[((w - 1) * 8 + k) * 64 + lane];
      float4* o = (float4*)(partials + (size_t)blockIdx.y * N + oct * 8);
      o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
  }
}

bool gelu_shape_ok(long long M, int N) {
  return M >= 1 && N >= 8 && N <= kGeluMaxN && N % 8 == 0;
}

#define GELU_DISPATCH_T(DT, ...)                                        \
  switch (DT) {                                                         \
    case DT_F32: { using scalar_t = float; __VA_ARGS__; break; }        \
    case DT_F16: { using scalar_t = __half; __VA_ARGS__; break; }       \
    case DT_BF16: { using scalar_t = __hip_bfloat16; __VA_ARGS__; break; } \
    default: return hipErrorInvalidValue;                               \
  }

#define GELU_DISPATCH_B(B, NAME, ...)                     \
  if (B) { constexpr bool NAME = true; __VA_ARGS__; }     \
  else { constexpr bool NAME = false; __VA_ARGS__; }

dim3 gelu_grid(int N, int chunks) {
  return dim3((unsigned)((N + kGeluTile - 1) / kGeluTile), (unsigned)chunks);
}

}  // namespace

// Row chunks of a launch, forward and backward alike.
//
// Every chunk costs one partial row in the backward: N floats written by the
// kernel and read again by the fold, 4 + 4 B per column, next to the rows * s
// bytes per column of dy the chunk reads (s = 2 or 4).  A chunk never has
// fewer than kGeluMinRows = 16 rows, so the kernel writes at most 4 / (16 *
// s) of the dy bytes as partial rows, 1/8 for fp16 / bf16 and 1/16 for fp32,
// and the fold reads as much.  Only launches of fewer than 16 * 1024 / tiles
// rows pay that much, and they want the blocks more than the bytes: at the
// benchmark's 1024 x 4096 (bf16, p = 0.1, measured on an MI355X, backward +
// fold) 16 rows per chunk, 512 blocks, take 10.2 us, 32 rows 10.8 us, 64 rows
// 14.9 us and 8 rows 10.1 us, no better for twice the partial rows.
// Larger launches stop at kGeluMaxBlocks = 1024 blocks, 4 per CU, which the
// instantiations of up to 128 VGPRs keep resident at once (two bias-gradient
// ones are just above); 16384 x 4096 then runs 128
// chunks of 128 rows with partial rows of 1/64 of the dy bytes.  The cap is a
// compromise between the two large shapes measured: 8192 x 3072 (6 column
// tiles) takes 33 us at 768 blocks and 40 us at 384, while 16384 x 4096 takes
// 94 us at 1024 blocks, 97 us at 2048 and 83 us at 512.
int GeluRowChunks(long long M, int N) {
  constexpr long long kGeluMinRows = 16, kGeluMaxBlocks = 1024;
  const long long tiles = (N + kGeluTile - 1) / kGeluTile;
  const long long by_rows = (M + kGeluMinRows - 1) / kGeluMinRows;
  const long long by_grid = std::max<long long>(1, kGeluMaxBlocks / tiles);
  return (int)std::max<long long>(1, std::min(by_rows, by_grid));
}

hipError_t GeluForwardLaunch(const void* u, const void* bias, bool bias_f32,
                             void* out, long long M, int N, int dt, bool tanh,
                             const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {u, bias, out};
  if (!gelu_shape_ok(M, N) || !u || !out || !aligned_to(ptrs, 3, 16))
    return hipErrorInvalidValue;
  const dim3 grid = gelu_grid(N, GeluRowChunks(M, N));
  GELU_DISPATCH_T(dt, GELU_DISPATCH_B(tanh, TANH,
      GELU_DISPATCH_B(d.t16 > 0, DROP,
      (gelu_fwd_k<scalar_t, TANH, DROP><<<grid, kGeluThreads, 0, stream>>>(
          (const scalar_t*)u, bias, bias_f32, (scalar_t*)out, M, N, d)))));
  return hipGetLastError();
}

hipError_t GeluBackwardLaunch(const void* dy, const void* u, const void* bias,
                              bool bias_f32, void* du, float* partials,
                              int chunks, long long M, int N, int dt,
                              bool tanh, const LnDropout& d,
                              hipStream_t stream) {
  const void* ptrs[] = {dy, u, bias, du, partials};
  if (!gelu_shape_ok(M, N) || !dy || !u || !du || !aligned_to(ptrs, 5, 16) ||
      chunks < 1 || chunks > 65535)
    return hipErrorInvalidValue;
  const dim3 grid = gelu_grid(N, chunks);
  const bool bg = partials != nullptr;
  GELU_DISPATCH_T(dt, GELU_DISPATCH_B(tanh, TANH,
      GELU_DISPATCH_B(d.t16 > 0, DROP, GELU_DISPATCH_B(bg, BG,
      (gelu_bwd_k<scalar_t, TANH, DROP, BG>
           <<<grid, kGeluThreads, 0, stream>>>(
          (const scalar_t*)dy, (const scalar_t*)u, bias, bias_f32,
          (scalar_t*)du, partials, M, N, d))))));
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
