// The dropout mask of the fused dropout + add + LayerNorm kernels
// (ln_kernels.hip).  The mask is never stored: forward, backward and the host
// evaluation behind fused_ln_keep_mask all call ln_keep8 below, so they cannot
// disagree.  docs/api.md carries the definition.
//
// Philox4x32-10 after Salmon, Moraes, Dror and Shaw, "Parallel random
// numbers: as easy as 1, 2, 3" (SC'11), written from the published algorithm.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace hvd {
namespace gpu {

// t16 == 0 keeps everything (p == 0), t16 == 65536 drops everything (p == 1).
struct LnDropout {
  unsigned long long seed = 0;
  unsigned long long offset = 0;
  unsigned int t16 = 0;
  float scale = 1.0f;  // 65536 / (65536 - t16); 0 when t16 == 65536
};

// p is quantised to 1/65536, nearest, ties away from zero
inline LnDropout LnMakeDropout(double p, unsigned long long seed,
                               unsigned long long offset) {
  long long t = std::llround(p * 65536.0);
  t = t < 0 ? 0 : (t > 65536 ? 65536 : t);
  LnDropout d;
  d.seed = seed;
  d.offset = offset;
  d.t16 = (unsigned int)t;
  d.scale = t == 65536 ? 0.0f : 65536.0f / (float)(65536 - t);
  return d;
}

// key = seed; counter = (v_lo, v_hi, offset_lo, offset_hi)
__host__ __device__ inline void ln_philox4x32_10(unsigned long long seed,
                                                 unsigned long long v,
                                                 unsigned long long offset,
                                                 uint32_t (&out)[4]) {
  uint32_t c0 = (uint32_t)v, c1 = (uint32_t)(v >> 32);
  uint32_t c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Bit k of the result is set iff element k of 8-element vector v is kept: the
// 128 output bits are eight 16-bit values, value k being bits [16 * (k % 2),
// 16 * (k % 2) + 16) of output word k / 2, and an element is kept iff its
// value >= t16.
__host__ __device__ inline unsigned int ln_keep8(const LnDropout& d,
                                                 unsigned long long v) {
  uint32_t w[4];
  ln_philox4x32_10(d.seed, v, d.offset, w);
  unsigned int keep = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t val = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
    keep |= (unsigned int)(val >= d.t16) << k;
  }
  return keep;
}

}  // namespace gpu
}  // namespace hvd
