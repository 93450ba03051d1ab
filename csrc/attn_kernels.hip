// Fused multi-head self-attention for the BERT encoder on the CDNA4 matrix
// instructions: forward and backward of
//   s_ij = 0.125 q_i . k_j,  p_i. = softmax_j(s_i.),  a_ij = keep_ij scale p_ij,
//   o_i = sum_j a_ij v_j
// straight on the packed in_proj output qkv [B, S, 3E] (q | k | v, head h in
// columns 64h .. 64h + 63 of each), head dimension 64, 1 <= S <= kAttnMaxS,
// fp16 or bf16.  out is [B, S, E] with the heads merged, dqkv is [B, S, 3E]
// and every element of it is written exactly once.
//
// All three kernels use v_mfma_f32_16x16x32_{f16,bf16}.  With l the lane,
// c = l % 16 and g = l / 16, the operands of D = A B + C (A 16x32, B 32x16)
// sit as follows: a lane holds the eight values A[c][8g .. 8g + 7], the eight
// values B[8g .. 8g + 7][c] and the four values D[4g .. 4g + 3][c].
//
// Forward and dQ (one block per batch, head and tile of 64 queries; a wave
// owns 16 queries against all keys) compute the TRANSPOSED scores
// S^T = K Q^T: K rows come from LDS as A, the wave's Q rows stay in registers
// as B.  MFMA row r of sub-tile t is given key 8 (r / 4) + 4 t + r % 4 of a
// group of 32 keys, so after two sub-tiles lane (c, g) holds the scores of
// query c against the eight consecutive keys 8g .. 8g + 7 of the group.
// That is one ln_keep8 octet of the dropout mask (one Philox call per eight
// probabilities), and it is the B layout of the second product O^T += V^T P^T
// (and dQ^T += K^T dS^T), whose A comes from a transposed copy of the tile in
// LDS.  P and dS never pass through LDS, all row statistics of a query live
// in the four lanes c, c + 16, c + 32, c + 48, and every accumulator element
// of a lane belongs to query c, so the online-softmax rescale is one scalar
// per lane.
//
// dK/dV (one block per batch, head and tile of 64 keys; a wave owns 16 keys
// against all queries) sums over queries, so it computes S = Q K^T with the
// same row trick applied to the queries: lane (c, g) holds key c against
// queries 8g .. 8g + 7, the B layout of dV^T += dO^T A and dK^T += Q^T dS.
// There an octet of the mask (one query, eight keys) is spread over eight
// lanes: lane (c, g) evaluates query 8g + c % 8 for the octet of its key and
// the lanes exchange the bits.  Q and dO tiles sit in LDS twice, row-major
// for the first products and transposed for the second.
//
// Nothing is accumulated across blocks: no atomics, no workspace but D_i =
// do_i . o_i (written by the dQ kernel, which runs first), results bitwise
// reproducible.  Loads of rows past S - 1 are clamped to row S - 1, their
// scores are excluded (-inf, or p = 0) and their stores predicated off.  A
// row with no allowed key has l = 0: out = 0, lse = -inf, and p = 0 by
// selection in the backward, so no inf - inf is ever formed.
#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kAttnThreads = 256;
constexpr int kAttnTile = 64;   // queries or keys of a block, keys of a step
constexpr int kAttnD = 64;      // head dimension
// LDS row pitch in elements: 144 B keeps the 16-B reads of 16 rows off one
// another's banks and stays 16-B aligned
constexpr int kAttnPitch = 72;
constexpr float kLog2e = 1.4426950408889634f;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma<__half>(const uint4& a, const uint4& b,
                                              f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(
      __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma<__hip_bfloat16>(const uint4& a,
                                                      const uint4& b,
                                                      f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// four elements, one 8-byte access
template <typename T>
union Vec4 {
  uint2 u;
  T e[4];
  __device__ Vec4() {}
};

// An LDS tile of 64 rows; raw 16-bit words, since T has constructors
#define ATTN_LDS_TILE(NAME)                                                  \
  __shared__ __attribute__((aligned(16))) unsigned short NAME##_w[kAttnTile * \
                                                                 kAttnPitch]; \
  T* const NAME = (T*)NAME##_w

// where a block works: grid = (tiles, heads, B)
struct AttnPos {
  int lane, wave, c, g;  // c = lane % 16, g = lane / 16
  int h, b, t0;          // head, batch entry, first row of the block's tile
};
__device__ __forceinline__ AttnPos attn_pos() {
  AttnPos p;
  p.lane = threadIdx.x & 63;
  p.wave = threadIdx.x >> 6;
  p.c = p.lane & 15;
  p.g = p.lane >> 4;
  p.h = blockIdx.y;
  p.b = blockIdx.z;
  p.t0 = blockIdx.x * kAttnTile;
  return p;
}

// the MFMA row trick: the tile row that row c of sub-tile t of group grp reads
__device__ __forceinline__ int attn_row(int grp, int t, int c) {
  return grp * 32 + 8 * (c >> 2) + 4 * t + (c & 3);
}

// The 64 x 64 tile of rows row0 .. row0 + 63 (clamped to S - 1) of one head:
// src points at column 0 of the head in row 0 of the batch entry, ld is the
// row pitch in elements.  rm: row-major copy, tr: transposed copy, either may
// be null.  512 16-B loads, two per thread.
template <typename T>
__device__ __forceinline__ void attn_load_tile(const T* __restrict__ src,
                                               size_t ld, int row0, int S,
                                               T* rm, T* tr) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = threadIdx.x + it * kAttnThreads;
    const int r = idx >> 3, ch = idx & 7;
    const int row = min(row0 + r, S - 1);
    Vec8<T> v;
    v.u[0] = *(const uint4*)(src + (size_t)row * ld + ch * 8);
    if (rm) *(uint4*)(rm + r * kAttnPitch + ch * 8) = v.u[0];
    if (tr) {
#pragma unroll
      for (int k = 0; k < 8; ++k) tr[(ch * 8 + k) * kAttnPitch + r] = v.e[k];
    }
  }
}

// B-operand fragments of row `row` (clamped) of a head: d = 8g + 32kc ..
template <typename T>
__device__ __forceinline__ void attn_load_frag(uint4 (&f)[2],
                                               const T* __restrict__ src,
                                               size_t ld, int row, int S,
                                               int g) {
  const T* p = src + (size_t)min(row, S - 1) * ld + 8 * g;
  f[0] = *(const uint4*)p;
  f[1] = *(const uint4*)(p + 32);
}

// rows attn_row(grp, t, c) of a row-major LDS tile against fragment f
template <typename T>
__device__ __forceinline__ f32x4 attn_rows_dot(const T* rm, int grp, int t,
                                               const AttnPos& w,
                                               const uint4 (&f)[2]) {
  const T* p = rm + attn_row(grp, t, w.c) * kAttnPitch + 8 * w.g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma<T>(*(const uint4*)p, f[0], acc);
  acc = mfma<T>(*(const uint4*)(p + 32), f[1], acc);
  return acc;
}

// acc[db] += tr[16 db + c][32 grp + 8g ..] x b: the second product
template <typename T>
__device__ __forceinline__ void attn_accumulate(f32x4 (&acc)[4], const T* tr,
                                                int grp, const AttnPos& w,
                                                const float (&x)[8]) {
  Vec8<T> b;
#pragma unroll
  for (int k = 0; k < 8; ++k) b.e[k] = from_f<T>(x[k]);
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const T* p = tr + (16 * db + w.c) * kAttnPitch + grp * 32 + 8 * w.g;
    acc[db] = mfma<T>(*(const uint4*)p, b.u[0], acc[db]);
  }
}

// acc holds X^T[16 db + 4g + r][row]: row `row` of dst gets 4 x 8-byte stores
template <typename T>
__device__ __forceinline__ void attn_store_row(T* __restrict__ dst, size_t ld,
                                               int row, const AttnPos& w,
                                               const f32x4 (&acc)[4],
                                               float mul) {
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    Vec4<T> o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o.e[r] = from_f<T>(acc[db][r] * mul);
    *(uint2*)(dst + (size_t)row * ld + 16 * db + 4 * w.g) = o.u;
  }
}

// ok[j] = key j0 + j exists and is not padding
__device__ __forceinline__ void attn_key_ok(unsigned char* ok,
                                            const unsigned char* __restrict__ m,
                                            int b, int j0, int S) {
  if (threadIdx.x < kAttnTile) {
    const int j = j0 + threadIdx.x;
    ok[threadIdx.x] = j < S && !(m && m[(size_t)b * S + j]);
  }
}

// the sum / maximum of a value over the four lanes that share c
__device__ __forceinline__ float attn_sum4(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float attn_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}

// mask vector of (b, h, query i, key octet j / 8): see kernels.h
__device__ __forceinline__ unsigned int attn_keep8(const LnDropout& d,
                                                   const AttnPos& w, int H,
                                                   int S, int i, int j) {
  const unsigned long long row =
      ((unsigned long long)w.b * H + w.h) * S + (unsigned)i;
  return ln_keep8(d, row * (unsigned)((S + 7) / 8) + (unsigned)(j >> 3));
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_k(
    const T* __restrict__ qkv, const unsigned char* __restrict__ mask,
    T* __restrict__ out, float* __restrict__ lse, int S, int H, LnDropout d) {
  ATTN_LDS_TILE(Ks);
  ATTN_LDS_TILE(Vt);
  __shared__ __attribute__((aligned(8))) unsigned char ok[kAttnTile];
  const AttnPos w = attn_pos();
  const size_t E = (size_t)H * kAttnD, ld = 3 * E;
  const T* base = qkv + (size_t)w.b * S * ld + w.h * kAttnD;
  const int q = w.t0 + w.wave * 16 + w.c;
  uint4 qf[2];
  attn_load_frag(qf, base, ld, q, S, w.g);

  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < S; j0 += kAttnTile) {
    if (j0) __syncthreads();
    attn_load_tile<T>(base + E, ld, j0, S, Ks, nullptr);
    attn_load_tile<T>(base + 2 * E, ld, j0, S, nullptr, Vt);
    attn_key_ok(ok, mask, w.b, j0, S);
    __syncthreads();

    // sc[grp][k]: query c against key j0 + 32 grp + 8g + k
    float sc[2][8];
    float tmax = -INFINITY;
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      const uint2 okv = *(const uint2*)(ok + grp * 32 + 8 * w.g);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 s = attn_rows_dot<T>(Ks, grp, t, w, qf);
        const unsigned int okw = t ? okv.y : okv.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v =
              ((okw >> (8 * r)) & 0xFFu) ? 0.125f * s[r] : -INFINITY;
          sc[grp][4 * t + r] = v;
          tmax = fmaxf(tmax, v);
        }
      }
    }
    const float m_new = fmaxf(m, attn_max4(tmax));
    // no allowed key so far: every exponent below is -inf, never inf - inf
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = exp2f((m - m_use) * kLog2e);
    float rsum = 0.f;
#pragma unroll
    for (int grp = 0; grp < 2; ++grp)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sc[grp][k] = exp2f((sc[grp][k] - m_use) * kLog2e);
        rsum += sc[grp][k];
      }
    l = l * alpha + attn_sum4(rsum);
    m = m_new;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      if (DROP) {
        const unsigned int keep =
            attn_keep8(d, w, H, S, q, j0 + grp * 32 + 8 * w.g);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          sc[grp][k] = ((keep >> k) & 1u) ? sc[grp][k] * d.scale : 0.f;
      }
      attn_accumulate<T>(o, Vt, grp, w, sc[grp]);
    }
  }
  if (q < S) {
    attn_store_row<T>(out + (size_t)w.b * S * E + w.h * kAttnD, E, q, w, o,
                      l > 0.f ? 1.0f / l : 0.f);
    if (w.g == 0)
      lse[((size_t)w.b * H + w.h) * S + q] =
          l > 0.f ? m + __logf(l) : -INFINITY;
  }
}

// dQ, and D_i = do_i . o_i for the dK/dV kernel
template <typename T, bool DROP>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dq_k(
    const T* __restrict__ dout, const T* __restrict__ qkv,
    const T* __restrict__ out, const float* __restrict__ lse,
    const unsigned char* __restrict__ mask, T* __restrict__ dqkv,
    float* __restrict__ D, int S, int H, LnDropout d) {
  ATTN_LDS_TILE(Ks);
  ATTN_LDS_TILE(Kt);
  ATTN_LDS_TILE(Vs);
  __shared__ __attribute__((aligned(8))) unsigned char ok[kAttnTile];
  const AttnPos w = attn_pos();
  const size_t E = (size_t)H * kAttnD, ld = 3 * E;
  const T* base = qkv + (size_t)w.b * S * ld + w.h * kAttnD;
  const size_t obase = (size_t)w.b * S * E + w.h * kAttnD;
  const int q = w.t0 + w.wave * 16 + w.c;
  const size_t stat = ((size_t)w.b * H + w.h) * S + min(q, S - 1);
  uint4 qf[2], dof[2], of[2];
  attn_load_frag(qf, base, ld, q, S, w.g);
  attn_load_frag(dof, dout + obase, E, q, S, w.g);
  attn_load_frag(of, out + obase, E, q, S, w.g);
  float Dq = 0.f;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    Vec8<T> a, b;
    a.u[0] = dof[kc];
    b.u[0] = of[kc];
#pragma unroll
    for (int k = 0; k < 8; ++k) Dq = fmaf(to_f<T>(a.e[k]), to_f<T>(b.e[k]), Dq);
  }
  Dq = attn_sum4(Dq);
  if (q < S && w.g == 0) D[stat] = Dq;
  const float lq = lse[stat];

  f32x4 dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < S; j0 += kAttnTile) {
    if (j0) __syncthreads();
    attn_load_tile<T>(base + E, ld, j0, S, Ks, Kt);
    attn_load_tile<T>(base + 2 * E, ld, j0, S, Vs, nullptr);
    attn_key_ok(ok, mask, w.b, j0, S);
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      const uint2 okv = *(const uint2*)(ok + grp * 32 + 8 * w.g);
      unsigned int keep = 0xFFu;
      if (DROP) keep = attn_keep8(d, w, H, S, q, j0 + grp * 32 + 8 * w.g);
      float ds[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 s = attn_rows_dot<T>(Ks, grp, t, w, qf);
        const f32x4 dp = attn_rows_dot<T>(Vs, grp, t, w, dof);
        const unsigned int okw = t ? okv.y : okv.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 4 * t + r;
          const float p = ((okw >> (8 * r)) & 0xFFu)
                              ? exp2f((0.125f * s[r] - lq) * kLog2e) : 0.f;
          const float dpv = ((keep >> k) & 1u) ? dp[r] * d.scale : 0.f;
          ds[k] = p * (dpv - Dq);
        }
      }
      attn_accumulate<T>(dq, Kt, grp, w, ds);
    }
  }
  if (q < S)
    attn_store_row<T>(dqkv + (size_t)w.b * S * ld + w.h * kAttnD, ld, q, w, dq,
                      0.125f);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dkv_k(
    const T* __restrict__ dout, const T* __restrict__ qkv,
    const float* __restrict__ lse, const float* __restrict__ D,
    const unsigned char* __restrict__ mask, T* __restrict__ dqkv, int S, int H,
    LnDropout d) {
  ATTN_LDS_TILE(Qs);
  ATTN_LDS_TILE(Qt);
  ATTN_LDS_TILE(dOs);
  ATTN_LDS_TILE(dOt);
  // per query of the tile: lse (+inf past S - 1, so that p = 0 there) and D
  __shared__ __attribute__((aligned(16))) float lse_s[kAttnTile];
  __shared__ __attribute__((aligned(16))) float D_s[kAttnTile];
  const AttnPos w = attn_pos();
  const size_t E = (size_t)H * kAttnD, ld = 3 * E;
  const T* base = qkv + (size_t)w.b * S * ld + w.h * kAttnD;
  const T* dobase = dout + (size_t)w.b * S * E + w.h * kAttnD;
  const size_t stat = ((size_t)w.b * H + w.h) * S;
  const int key = w.t0 + w.wave * 16 + w.c;
  const bool key_ok = key < S && !(mask && mask[(size_t)w.b * S + key]);
  uint4 kf[2], vf[2];
  attn_load_frag(kf, base + E, ld, key, S, w.g);
  attn_load_frag(vf, base + 2 * E, ld, key, S, w.g);

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
    dk[db] = dv[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int i0 = 0; i0 < S; i0 += kAttnTile) {
    if (i0) __syncthreads();
    attn_load_tile<T>(base, ld, i0, S, Qs, Qt);
    attn_load_tile<T>(dobase, E, i0, S, dOs, dOt);
    if (threadIdx.x < kAttnTile) {
      const int i = i0 + threadIdx.x;
      lse_s[threadIdx.x] = i < S ? lse[stat + i] : INFINITY;
      D_s[threadIdx.x] = D[stat + min(i, S - 1)];
    }
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      // lane (c, g): key c of the wave against queries i0 + 32 grp + 8g + k
      const int qi = grp * 32 + 8 * w.g;
      unsigned int mine = 0xFFu;
      if (DROP) mine = attn_keep8(d, w, H, S, i0 + qi + (w.c & 7), key);
      float a[8], ds[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 s = attn_rows_dot<T>(Qs, grp, t, w, kf);
        const f32x4 dp = attn_rows_dot<T>(dOs, grp, t, w, vf);
        const float4 lq = *(const float4*)(lse_s + qi + 4 * t);
        const float4 Dq = *(const float4*)(D_s + qi + 4 * t);
        const float lqa[4] = {lq.x, lq.y, lq.z, lq.w};
        const float Dqa[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 4 * t + r;
          // the octet of query 8g + k is with the lane whose c % 8 is k
          bool keep = true;
          if (DROP)
            keep = (__shfl(mine, (w.lane & ~7) | k, 64) >> (w.c & 7)) & 1u;
          // lqa = +inf past S - 1 and -inf for a row without keys (then
          // key_ok is false for every key of the sequence)
          const float p =
              key_ok ? exp2f((0.125f * s[r] - lqa[r]) * kLog2e) : 0.f;
          a[k] = keep ? p * d.scale : 0.f;
          ds[k] = p * ((keep ? dp[r] * d.scale : 0.f) - Dqa[r]);
        }
      }
      attn_accumulate<T>(dv, dOt, grp, w, a);
      attn_accumulate<T>(dk, Qt, grp, w, ds);
    }
  }
  if (key < S) {
    T* dst = dqkv + (size_t)w.b * S * ld + w.h * kAttnD;
    attn_store_row<T>(dst + E, ld, key, w, dk, 0.125f);
    attn_store_row<T>(dst + 2 * E, ld, key, w, dv, 1.0f);
  }
}

bool attn_shape_ok(long long B, int S, int H) {
  return B >= 1 && B <= 65535 && S >= 1 && S <= kAttnMaxS && H >= 1 &&
         H <= 65535;
}

dim3 attn_grid(long long B, int S, int H) {
  return dim3((unsigned)((S + kAttnTile - 1) / kAttnTile), (unsigned)H,
              (unsigned)B);
}

#define ATTN_DISPATCH(DT, DROPV, ...)                                    \
  switch (DT) {                                                          \
    case DT_F16: {                                                       \
      using scalar_t = __half;                                           \
      if (DROPV) { constexpr bool DROP = true; __VA_ARGS__; }            \
      else { constexpr bool DROP = false; __VA_ARGS__; }                 \
      break;                                                             \
    }                                                                    \
    case DT_BF16: {                                                      \
      using scalar_t = __hip_bfloat16;                                   \
      if (DROPV) { constexpr bool DROP = true; __VA_ARGS__; }            \
      else { constexpr bool DROP = false; __VA_ARGS__; }                 \
      break;                                                             \
    }                                                                    \
    default: return hipErrorInvalidValue;                                \
  }

}  // namespace

hipError_t AttnForwardLaunch(const void* qkv, const unsigned char* mask,
                             void* out, float* lse, long long B, int S, int H,
                             int dt, const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {qkv, out};
  if (!attn_shape_ok(B, S, H) || !qkv || !out || !lse ||
      !aligned_to(ptrs, 2, 16))
    return hipErrorInvalidValue;
  ATTN_DISPATCH(dt, d.t16 > 0,
      (attn_fwd_k<scalar_t, DROP>
           <<<attn_grid(B, S, H), kAttnThreads, 0, stream>>>(
          (const scalar_t*)qkv, mask, (scalar_t*)out, lse, S, H, d)));
  return hipGetLastError();
}

hipError_t AttnBackwardLaunch(const void* dout, const void* qkv,
                              const void* out, const float* lse,
                              const unsigned char* mask, void* dqkv, float* D,
                              long long B, int S, int H, int dt,
                              const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {dout, qkv, out, dqkv};
  if (!attn_shape_ok(B, S, H) || !dout || !qkv || !out || !lse || !dqkv ||
      !D || !aligned_to(ptrs, 4, 16))
    return hipErrorInvalidValue;
  const dim3 grid = attn_grid(B, S, H);
  ATTN_DISPATCH(dt, d.t16 > 0,
      (attn_bwd_dq_k<scalar_t, DROP><<<grid, kAttnThreads, 0, stream>>>(
          (const scalar_t*)dout, (const scalar_t*)qkv, (const scalar_t*)out,
          lse, mask, (scalar_t*)dqkv, D, S, H, d));
      (attn_bwd_dkv_k<scalar_t, DROP><<<grid, kAttnThreads, 0, stream>>>(
          (const scalar_t*)dout, (const scalar_t*)qkv, lse, D, mask,
          (scalar_t*)dqkv, S, H, d)));
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
