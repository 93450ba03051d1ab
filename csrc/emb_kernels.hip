// Fused embedding + LayerNorm + dropout for the BERT input block:
// row r = b * S + s of ids [B, S] is z = tok[ids_r] + pos[s] (+ typ[types_r]),
// y = keep * scale * (gamma * (z - mean) * rstd + beta).
//
// A row lives in registers with the decomposition of ln_kernels.hip (lane l
// holds the 8-element vectors l, l + 64 * WPR, ... of the row, one wave up to
// H = 1024, two up to 2048, four up to 4096).  The split of work is by
// position: the grid is position blocks x batch chunks, and the wave (or the
// WPR waves) that owns position s keeps pos[s], gamma and beta in registers
// and walks the batch entries of its chunk, so a row costs one gathered token
// row in and one row of y out; the type row comes from a table of at most two
// rows, which the cache holds.  The token rows of two batch entries are
// requested before the first is used.
//
// Nothing but mean and rstd is saved.  Backward pass one (emb_ln_bwd_k) walks
// the same way, gathers z again, and writes the gradient of z as fp32 rows
// dz [M, H].  Because the owner of position s sees every row of that
// position in its chunk, dpos[s], the per-type sums of dz and the two sums
// behind dgamma and dbeta all stay in registers over the walk and leave once:
// dpos as row `chunk` of [chunks, S, H], the other four as one partial row
// per block, both folded in a fixed order by ln_fold_k (ColumnFoldLaunch).
//
// Pass two (emb_scatter_k) is the token table's gradient, turned from a
// scatter into a gather: a wave owns token v, finds the segment of the stably
// sorted ids that equals v with a 64-way search (every lane probes one
// position, a ballot picks the sub-range: three rounds for 8192 rows), adds
// the dz rows of the segment in sorted order and writes row v, zeros where
// the segment is empty.  Every element of the [V, H] gradient is written
// exactly once: no memset, no atomics, no dependence on launch order.
#include "ln_common.h"

namespace hvd {
namespace gpu {
namespace {

// Batch entries whose loads are in flight together.  Forward: two token rows,
// with fp32 tables and two vectors per lane eight 16-B loads per lane, as in
// gelu_kernels.hip.  The backward also loads dy and holds four accumulators
// per element: one entry at a time keeps it at two waves per SIMD.
constexpr int kEmbFwdUnroll = 2;
constexpr int kEmbBwdUnroll = 1;

// row `row` of a table of H-element rows of fp32 or T
template <typename T>
__device__ __forceinline__ const void* emb_row(const void* p, bool f32,
                                               long long row, int H) {
  return (const char*)p +
         (size_t)row * H * ((f32 || sizeof(T) == 4) ? 4 : sizeof(T));
}

// 8 elements of a table row as they are loaded, fp32 (two 16-B loads) or T,
// and their conversion, apart so that loads can be issued ahead of their use
template <typename T>
__device__ __forceinline__ void emb_load(uint4 (&r)[2], const void* row,
                                         bool f32, int vi) {
  if (f32 || sizeof(T) == 4) {
    r[0] = ((const uint4*)row)[vi * 2];
    r[1] = ((const uint4*)row)[vi * 2 + 1];
  } else {
    r[0] = ((const uint4*)row)[vi];
    r[1] = r[0];
  }
}

template <typename T>
__device__ __forceinline__ void emb_cvt(float (&f)[8], const uint4 (&r)[2],
                                        bool f32) {
  if (f32 || sizeof(T) == 4) {
    f[0] = __uint_as_float(r[0].x); f[1] = __uint_as_float(r[0].y);
    f[2] = __uint_as_float(r[0].z); f[3] = __uint_as_float(r[0].w);
    f[4] = __uint_as_float(r[1].x); f[5] = __uint_as_float(r[1].y);
    f[6] = __uint_as_float(r[1].z); f[7] = __uint_as_float(r[1].w);
  } else {
    Vec8<T> v;
    v.u[0] = r[0];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = to_f<T>(v.e[k]);
  }
}

// Token id and type of row `row`, clamped into their tables; false when
// either was outside, which makes the row NaN and keeps it out of every
// gradient.
__device__ __forceinline__ bool emb_index(const EmbTables& t, long long row,
                                          long long& id, int& tt) {
  id = t.ids[row];
  bool ok = id >= 0 && id < t.V;
  id = min(max(id, 0LL), t.V - 1);
  tt = 0;
  if (t.types) {
    const long long ty = t.types[row];
    ok = ok && ty >= 0 && ty < t.ntypes;
    tt = (int)min(max(ty, 0LL), (long long)t.ntypes - 1);
  }
  return ok;
}

// The batch entries [b0, b1) of chunk blockIdx.y: ceil(B / gridDim.y) each,
// the last ones shorter or empty.
__device__ __forceinline__ void emb_chunk(int B, int& b0, int& b1) {
  const int bpc = (B + gridDim.y - 1) / gridDim.y;
  b0 = min(B, (int)blockIdx.y * bpc);
  b1 = min(B, b0 + bpc);
}

// Vector i of a lane is vector emb_vi(i) of its row, and the lane's waves own
// position emb_pos().
template <int WPR>
__device__ __forceinline__ int emb_vi(int i) {
  return (i * WPR + (threadIdx.x >> 6) % WPR) * 64 + (threadIdx.x & 63);
}

template <int WPR>
__device__ __forceinline__ int emb_pos() {
  return blockIdx.x * (kLnWaves / WPR) + (threadIdx.x >> 6) / WPR;
}

// vector i of the lane exists: inside the row, at a position inside S
#define EMB_ON(i) (s < t.S && emb_vi<WPR>(i) < t.H / 8)

// What the owner of position s holds for the whole walk: pos[s] and gamma.  A
// vector that does not exist reads the last one that does, and is not used.
template <typename T, int NV, int WPR>
__device__ __forceinline__ void emb_owner(float (&pz)[NV][8],
                                          float (&ga)[NV][8],
                                          const EmbTables& t) {
  const void* prow =
      emb_row<T>(t.pos, t.pos_f32, min(emb_pos<WPR>(), t.S - 1), t.H);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = min(emb_vi<WPR>(i), t.H / 8 - 1);
    ln_param8<T>(pz[i], prow, t.pos_f32, vi, 0.f);
    ln_param8<T>(ga[i], t.gamma, t.gamma_f32, vi, 1.f);
  }
}

// z of NR batch entries b, b + 1, ... at the owner's position: every token
// row is requested before the first is converted.  ok[j]: both indices of
// entry j were inside their tables.
template <typename T, int NV, int WPR, int NR>
__device__ __forceinline__ void emb_gather(const float (&pz)[NV][8],
                                           const EmbTables& t, int b,
                                           float (&z)[NR][NV][8],
                                           bool (&ok)[NR], int (&tt)[NR]) {
  const int s = emb_pos<WPR>();
  uint4 raw[NR][NV][2];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    long long id = 0;
    tt[j] = 0;
    ok[j] = false;
    if (s < t.S)
      ok[j] = emb_index(t, (long long)(b + j) * t.S + s, id, tt[j]);
    const void* row = emb_row<T>(t.tok, t.tok_f32, id, t.H);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (EMB_ON(i)) emb_load<T>(raw[j][i], row, t.tok_f32, emb_vi<WPR>(i));
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const void* trow = emb_row<T>(t.typ, t.typ_f32, tt[j], t.H);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (EMB_ON(i)) {
        float tk[8], ty[8];
        emb_cvt<T>(tk, raw[j][i], t.tok_f32);
        ln_param8<T>(ty, t.types ? trow : nullptr, t.typ_f32, emb_vi<WPR>(i),
                     0.f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          z[j][i][k] = tk[k] + pz[i][k];
          if (t.types) z[j][i][k] += ty[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) z[j][i][k] = 0.f;
      }
    }
  }
}

template <typename T, int NV, int WPR, bool DROP, int NR>
__device__ __forceinline__ void emb_fwd_rows(
    const float (&pz)[NV][8], const float (&ga)[NV][8],
    const float (&be)[NV][8], const EmbTables& t,
    int b, T* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd, float eps, const LnDropout& d, float* red) {
  const int vpr = t.H / 8;
  const int s = emb_pos<WPR>();
  const float inv_h = 1.0f / (float)t.H;
  float z[NR][NV][8];
  bool ok[NR];
  int tt[NR];
  emb_gather<T, NV, WPR, NR>(pz, t, b, z, ok, tt);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long row = (long long)(b + j) * t.S + s;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) sum += z[j][i][k];
    const float m = ln_row_sum<WPR>(sum, red) * inv_h;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (EMB_ON(i)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float c = z[j][i][k] - m;
          q += c * c;
        }
      }
    }
    const float rs = rsqrtf(ln_row_sum<WPR>(q, red) * inv_h + eps);
    if (s < t.S && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) % WPR == 0) {
      mean[row] = m;
      rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (EMB_ON(i)) {
        const long long v = row * vpr + emb_vi<WPR>(i);
        unsigned int keep = 0xFFu;
        if (DROP) keep = ln_keep8(d, (unsigned long long)v);
        Vec8<T> yv;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float f = (z[j][i][k] - m) * rs * ga[i][k] + be[i][k];
          if (DROP) f = ((keep >> k) & 1u) ? f * d.scale : 0.f;
          yv.e[k] = from_f<T>(ok[j] ? f : __builtin_nanf(""));
        }
        store8(y, v, yv);
      }
    }
  }
}

// grid: (position blocks, batch chunks).  Every thread of a block walks the
// same batch entries, so the barriers of ln_row_sum are met by all of them.
template <typename T, int NV, int WPR, bool DROP>
__global__ __launch_bounds__(kLnThreads) void emb_ln_fwd_k(
    EmbTables t, T* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd, float eps, LnDropout d) {
  __shared__ float red[kLnWaves];
  float pz[NV][8], ga[NV][8], be[NV][8];
  emb_owner<T, NV, WPR>(pz, ga, t);
#pragma unroll
  for (int i = 0; i < NV; ++i)
    ln_param8<T>(be[i], t.beta, t.beta_f32,
                 min(emb_vi<WPR>(i), t.H / 8 - 1), 0.f);
  int b, b1;
  emb_chunk(t.B, b, b1);
  for (; b + kEmbFwdUnroll <= b1; b += kEmbFwdUnroll)
    emb_fwd_rows<T, NV, WPR, DROP, kEmbFwdUnroll>(pz, ga, be, t, b, y, mean,
                                                  rstd, eps, d, red);
  for (; b < b1; ++b)
    emb_fwd_rows<T, NV, WPR, DROP, 1>(pz, ga, be, t, b, y, mean, rstd, eps, d,
                                      red);
}

// The owner's sums over its walk: ag = sum g xhat and ab = sum g with g = dy
// * keep * scale (dgamma, dbeta), and d0 / d1 = the sums of dz over the rows
// of type 0 / 1 (everything is type 0 without types).  dpos[s] is d0 + d1.
template <typename T, int NV, int WPR, bool DROP, bool TYPES, int NR>
__device__ __forceinline__ void emb_bwd_rows(
    const float (&pz)[NV][8], const float (&ga)[NV][8],
    float (&ag)[NV][8], float (&ab)[NV][8], float (&d0)[NV][8],
    float (&d1)[NV][8], const EmbTables& t, int b,
    const T* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dz,
    const LnDropout& d, float* red) {
  const int vpr = t.H / 8;
  const int s = emb_pos<WPR>();
  const float inv_h = 1.0f / (float)t.H;
  Vec8<T> dv[NR][NV];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (EMB_ON(i))
        load8(dv[j][i], dy,
              ((long long)(b + j) * t.S + s) * vpr + emb_vi<WPR>(i));
  float z[NR][NV][8];
  bool ok[NR];
  int tt[NR];
  emb_gather<T, NV, WPR, NR>(pz, t, b, z, ok, tt);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long row = (long long)(b + j) * t.S + s;
    const float m = s < t.S ? mean[row] : 0.f;
    const float rs = s < t.S ? rstd[row] : 0.f;
    float g[NV][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (EMB_ON(i)) {
        unsigned int keep = 0xFFu;
        const long long v = row * vpr + emb_vi<WPR>(i);
        if (DROP) keep = ln_keep8(d, (unsigned long long)v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          g[i][k] = to_f<T>(dv[j][i].e[k]);
          if (DROP) g[i][k] = ((keep >> k) & 1u) ? g[i][k] * d.scale : 0.f;
          z[j][i][k] = (z[j][i][k] - m) * rs;  // xhat from here on
          const float gg = g[i][k] * ga[i][k];
          s1 += gg;
          s2 += gg * z[j][i][k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) g[i][k] = 0.f;
      }
    }
    const float a = ln_row_sum<WPR>(s1, red) * inv_h;
    const float c = ln_row_sum<WPR>(s2, red) * inv_h;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (EMB_ON(i)) {
        float dzf[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float xh = z[j][i][k];
          dzf[k] = ok[j] ? rs * (g[i][k] * ga[i][k] - a - xh * c) : 0.f;
          if (ok[j]) {
            ag[i][k] += g[i][k] * xh;
            ab[i][k] += g[i][k];
          }
          const float to1 = (TYPES && tt[j] == 1) ? dzf[k] : 0.f;
          d1[i][k] += to1;
          d0[i][k] += dzf[k] - to1;
        }
        float4* out = (float4*)dz + (row * vpr + emb_vi<WPR>(i)) * 2;
        out[0] = make_float4(dzf[0], dzf[1], dzf[2], dzf[3]);
        out[1] = make_float4(dzf[4], dzf[5], dzf[6], dzf[7]);
      }
    }
  }
}

// Same grid and ownership as the forward.  wpart row blockIdx.y * gridDim.x +
// blockIdx.x is [ag, ab(, dt0, dt1)] of H floats each; the position owners
// of a block (more than one up to H = 2048) meet in the dynamic LDS of that
// size, added in rising wave order.
template <typename T, int NV, int WPR, bool DROP, bool TYPES>
__global__ __launch_bounds__(kLnThreads) void emb_ln_bwd_k(
    EmbTables t, const T* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dz,
    float* __restrict__ dpos_part, float* __restrict__ wpart, LnDropout d) {
  extern __shared__ float4 emb_lds[];
  __shared__ float red[kLnWaves];
  constexpr int PPB = kLnWaves / WPR;
  constexpr int NACC = TYPES ? 4 : 2;
  const int H = t.H;
  const int s = emb_pos<WPR>();
  float pz[NV][8], ga[NV][8], ag[NV][8], ab[NV][8], d0[NV][8], d1[NV][8];
  emb_owner<T, NV, WPR>(pz, ga, t);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ag[i][k] = ab[i][k] = d0[i][k] = d1[i][k] = 0.f;
    }
  int b, b1;
  emb_chunk(t.B, b, b1);
  for (; b + kEmbBwdUnroll <= b1; b += kEmbBwdUnroll)
    emb_bwd_rows<T, NV, WPR, DROP, TYPES, kEmbBwdUnroll>(
        pz, ga, ag, ab, d0, d1, t, b, dy, mean, rstd, dz, d, red);
  for (; b < b1; ++b)
    emb_bwd_rows<T, NV, WPR, DROP, TYPES, 1>(pz, ga, ag, ab, d0, d1, t, b, dy,
                                             mean, rstd, dz, d, red);

  float* out =
      wpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NACC * H;
  float* lds = (float*)emb_lds;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!EMB_ON(i)) continue;
    float dp[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      dp[k] = TYPES ? d0[i][k] + d1[i][k] : d0[i][k];
    float4* p = (float4*)(dpos_part + ((size_t)blockIdx.y * t.S + s) * H) +
                emb_vi<WPR>(i) * 2;
    p[0] = make_float4(dp[0], dp[1], dp[2], dp[3]);
    p[1] = make_float4(dp[4], dp[5], dp[6], dp[7]);
  }
  // a position past S holds zeros and owns the same columns as the others
#pragma unroll
  for (int r = 0; r < PPB; ++r) {
    if ((int)(threadIdx.x >> 6) / WPR == r) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int vi = emb_vi<WPR>(i);
        if (vi >= H / 8) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = vi * 8 + k;
          float* dst = PPB == 1 ? out : lds;
          if (r == 0) {
            dst[c] = ag[i][k];
            dst[H + c] = ab[i][k];
            if (TYPES) {
              dst[2 * H + c] = d0[i][k];
              dst[3 * H + c] = d1[i][k];
            }
          } else {
            dst[c] += ag[i][k];
            dst[H + c] += ab[i][k];
            if (TYPES) {
              dst[2 * H + c] += d0[i][k];
              dst[3 * H + c] += d1[i][k];
            }
          }
        }
      }
    }
    if (PPB > 1) __syncthreads();
  }
  if (PPB > 1)
    for (int c = threadIdx.x; c < NACC * H; c += kLnThreads) out[c] = lds[c];
}

// First index of a[0, n) that is not below key (n if none), found by the
// whole wave: lane l probes the end of the l-th of 64 equal parts of the
// range, and since a is sorted the lanes that see a smaller value are a
// prefix, whose length picks the part to go on with.
__device__ __forceinline__ long long emb_lower_bound(
    const long long* __restrict__ a, long long lo, long long n,
    long long key) {
  const int lane = threadIdx.x & 63;
  while (n > 0) {
    const long long step = (n + 63) / 64;
    const long long off = (lane + 1) * step - 1;
    const bool less = off < n && a[lo + off] < key;
    const long long cnt = __popcll(__ballot(less));
    const long long end = lo + n;
    lo += cnt * step;
    n = min(step - 1, end - lo);
  }
  return lo;
}

// One wave per token v < V, then one per row [S, P) of dpos, which no
// position owner of pass one wrote.
__global__ __launch_bounds__(kLnThreads) void emb_scatter_k(
    const long long* __restrict__ sorted_ids, const long long* __restrict__ perm,
    const float* __restrict__ dz, float* __restrict__ dtok,
    float* __restrict__ dpos, long long M, int H, long long V, int S, int P) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * kLnWaves + (threadIdx.x >> 6);
  const int vpr = H / 8;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (w >= V) {
    if (w - V >= P - S) return;
    float4* out = (float4*)(dpos + (size_t)(S + (w - V)) * H);
    for (int i = lane; i < 2 * vpr; i += 64) out[i] = zero;
    return;
  }
  const long long lo = emb_lower_bound(sorted_ids, 0, M, w);
  const long long hi = emb_lower_bound(sorted_ids, lo, M - lo, w + 1);
  float4* out = (float4*)(dtok + (size_t)w * H);
  // 128 vectors of the row per round, two per lane
  for (int v0 = lane; v0 < vpr; v0 += 128) {
    const bool two = v0 + 64 < vpr;
    float4 a[4] = {zero, zero, zero, zero};
    auto add = [&](const float4 (&r)[4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q].x += r[q].x; a[q].y += r[q].y;
        a[q].z += r[q].z; a[q].w += r[q].w;
      }
    };
    auto load = [&](float4 (&r)[4], long long j) {
      const float4* row = (const float4*)(dz + (size_t)perm[j] * H);
      r[0] = row[v0 * 2];
      r[1] = row[v0 * 2 + 1];
      r[2] = two ? row[(v0 + 64) * 2] : zero;
      r[3] = two ? row[(v0 + 64) * 2 + 1] : zero;
    };
    long long j = lo;
    for (; j + 1 < hi; j += 2) {
      float4 r0[4], r1[4];
      load(r0, j);
      load(r1, j + 1);
      add(r0);
      add(r1);
    }
    if (j < hi) {
      float4 r0[4];
      load(r0, j);
      add(r0);
    }
    out[v0 * 2] = a[0];
    out[v0 * 2 + 1] = a[1];
    if (two) {
      out[(v0 + 64) * 2] = a[2];
      out[(v0 + 64) * 2 + 1] = a[3];
    }
  }
}

bool emb_args_ok(const EmbTables& t) {
  const void* ptrs[] = {t.ids, t.types, t.tok, t.pos, t.typ, t.gamma, t.beta};
  return t.ids && t.tok && t.pos && t.B >= 1 && t.S >= 1 && t.S <= t.P &&
         t.V >= 1 && t.H >= 8 && t.H <= kLnMaxH && t.H % 8 == 0 &&
         (!t.types || (t.typ && t.ntypes >= 1 && t.ntypes <= kEmbMaxTypes)) &&
         aligned_to(ptrs + 2, 5, 16) && aligned_to(ptrs, 2, 8);
}

dim3 emb_grid(const EmbTables& t, int chunks) {
  return dim3((unsigned)EmbPositionBlocks(t.S, t.H), (unsigned)chunks);
}

}  // namespace

int EmbPositionBlocks(int S, int H) {
  const int ppb = kLnWaves / ln_waves_per_row(H);
  return (S + ppb - 1) / ppb;
}

// Batch chunks of a launch.  A chunk of the forward costs its owner one more
// load of pos[s], gamma and beta; a chunk of the backward also one more row
// of dpos partials (H floats written and folded again next to the walk's rows
// of 4 H bytes of dz each) and one more partial row of the parameter sums
// per block.  So the chunks stop at kEmbBlocks = 512 blocks, two per compute
// unit, and no chunk walks fewer than 4 batch entries forward (the partial
// traffic is nil there) or 8 backward (dpos partials at most 1/8 of the dz
// bytes).  The benchmark's 64 x 128 ids at H = 1024 run 32 position blocks x
// 16 chunks forward and x 8 backward; 16 x 512 runs 128 x 4 and 128 x 2.
int EmbBatchChunks(int B, int S, int H, bool backward) {
  constexpr int kEmbBlocks = 512;
  const int min_walk = backward ? 8 : 4;
  const int posblocks = EmbPositionBlocks(S, H);
  const int by_walk = (B + min_walk - 1) / min_walk;
  const int by_grid = (kEmbBlocks + posblocks - 1) / posblocks;
  return std::max(1, std::min(std::min(by_walk, by_grid), 65535));
}

hipError_t EmbForwardLaunch(const EmbTables& t, void* y, float* mean,
                            float* rstd, int dt, float eps,
                            const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {y};
  if (!emb_args_ok(t) || !y || !mean || !rstd || !aligned_to(ptrs, 1, 16))
    return hipErrorInvalidValue;
  const dim3 grid = emb_grid(t, EmbBatchChunks(t.B, t.S, t.H, false));
  LN_DISPATCH_T(dt, LN_DISPATCH_H(t.H, LN_DISPATCH_B(d.t16 > 0, DROP,
      (emb_ln_fwd_k<scalar_t, NV, WPR, DROP><<<grid, kLnThreads, 0, stream>>>(
          t, (scalar_t*)y, mean, rstd, eps, d)))));
  return hipGetLastError();
}

hipError_t EmbBackwardLaunch(const EmbTables& t, const void* dy,
                             const float* mean, const float* rstd, float* dz,
                             float* dpos_part, float* wpart, int chunks,
                             int dt, const LnDropout& d, hipStream_t stream) {
  const void* ptrs[] = {dy, dz, dpos_part, wpart};
  if (!emb_args_ok(t) || !dy || !mean || !rstd || !dz || !dpos_part ||
      !wpart || !aligned_to(ptrs, 4, 16) || chunks < 1 || chunks > 65535)
    return hipErrorInvalidValue;
  const dim3 grid = emb_grid(t, chunks);
  const bool types = t.types != nullptr;
  const size_t lds = ln_waves_per_row(t.H) == kLnWaves
                         ? 0
                         : (size_t)(types ? 4 : 2) * t.H * sizeof(float);
  LN_DISPATCH_T(dt, LN_DISPATCH_H(t.H, LN_DISPATCH_B(d.t16 > 0, DROP,
      LN_DISPATCH_B(types, TYPES,
      (emb_ln_bwd_k<scalar_t, NV, WPR, DROP, TYPES>
           <<<grid, kLnThreads, lds, stream>>>(
          t, (const scalar_t*)dy, mean, rstd, dz, dpos_part, wpart, d))))));
  return hipGetLastError();
}

hipError_t EmbScatterLaunch(const long long* sorted_ids,
                            const long long* perm, const float* dz,
                            float* dtok, float* dpos, long long M, int H,
                            long long V, int S, int P, hipStream_t stream) {
  const void* ptrs[] = {dz, dtok, dpos};
  if (!sorted_ids || !perm || !dz || !dtok || !dpos || M < 1 || V < 1 ||
      S < 1 || S > P || H < 8 || H > kLnMaxH || H % 8 != 0 ||
      !aligned_to(ptrs, 3, 16))
    return hipErrorInvalidValue;
  const long long blocks = (V + (P - S) + kLnWaves - 1) / kLnWaves;
  if (blocks >= (1LL << 31)) return hipErrorInvalidValue;
  emb_scatter_k<<<(unsigned)blocks, kLnThreads, 0, stream>>>(
      sorted_ids, perm, dz, dtok, dpos, M, H, V, S, P);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
