// Device helpers shared by the multi-tensor kernels that divide work by
// fixed element chunks (clip_kernels.hip, lamb_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace hvd {
namespace gpu {

constexpr int kClipThreads = 256;

struct ChunkRef {
  int tensor;
  long long begin;  // element range of this block within the tensor
  long long end;
};

// Largest t with block_prefix[t] <= blockIdx.x (block_prefix[count] is the
// grid size, so the invariant prefix[lo] <= b < prefix[hi] always holds).
// Args: a by-value kernel argument with count, numel[] and block_prefix[].
template <typename Args>
__device__ __forceinline__ ChunkRef find_chunk(const Args& args) {
  const unsigned int b = blockIdx.x;
  int lo = 0, hi = args.count;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (args.block_prefix[mid] <= b) lo = mid; else hi = mid;
  }
  ChunkRef c;
  c.tensor = lo;
  c.begin = (long long)(b - args.block_prefix[lo]) * kClipChunk;
  const long long n = (long long)args.numel[lo];
  c.end = c.begin + kClipChunk < n ? c.begin + kClipChunk : n;
  return c;
}

// Sum over the block in a fixed order: wave64 shuffle tree, then the wave
// leaders through LDS.  Valid in thread 0.
__device__ __forceinline__ float block_sum(float v) {
  __shared__ float wave_part[kClipThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  float total = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kClipThreads / 64; ++w) total += wave_part[w];
  }
  return total;
}

}  // namespace gpu
}  // namespace hvd
