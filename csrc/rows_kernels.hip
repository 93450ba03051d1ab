// Row compaction for the BERT MLM head: the positions of the labelled rows of
// labels [M] (label != ignore_index), the gather of those rows of x [M, H]
// into rows [capacity, H], and the gather's backward.  Nothing is read by the
// host, nothing is cleared by a memset, there are no atomics, and no block
// ever waits for another block of its launch.
//
// Index build (rows_index_k).  A block owns one chunk of kRowsChunk = 2048
// labels: each of its 256 threads has kRowsLoads = 4 16-B loads of two labels
// in flight, load j of thread t being the label pair j * 256 + t of the chunk,
// so a wave reads 1 KB in a row.  In position order the chunk is therefore
// cut into 16 segments (j, wave) of 128 labels.  Inside a segment a lane
// ranks its pair with two ballots (one per element of the pair) and
// popcounts below its own bit; the segments' counts meet in LDS, and every
// thread adds those before its own.  The block's base is the number of
// labelled rows in the chunks before it: either the sum of the per-chunk
// counts that rows_count_k wrote in a launch before this one (COUNTS), or the
// block counts the labels of those chunks itself, again four loads in flight
// (one launch; chunk c reads c chunks, so this is for short arrays only).
// The block of the last chunk knows the total: it writes count and the tails
// [count, capacity) of idx (-1) and row_labels (ignore_index).
//
// Gather (rows_gather_k).  Pure 16-B copies, so one instantiation serves
// every dtype; the host passes the NaN pattern as a 32-bit word.  A block is
// one wave and owns kRowsGatherRows = 4 consecutive rows of the output.  Its
// source positions and the count are block-uniform loads that end as scalar
// registers, and the lanes walk the row's vectors with the loads of all four
// rows requested before the first store.  A row at or past count is zeros;
// with count > capacity every row is NaN, as is a row whose position is
// outside [0, M) (never written by rows_index_k, but idx is an argument).
//
// Scatter (rows_scatter_k).  One pass over dx [M, H] in the cl-vec8
// decomposition of the BatchNorm kernels (grid_for): a thread owns one 16-B
// column vector and walks down the rows, kRowsScatterRows = 4 rows at a time:
// four ranks, then four loads from d_rows (or zeros), then four stores.
// Every vector of dx is stored exactly once.
#include "bn_common.h"

namespace hvd {
namespace gpu {
namespace {

constexpr int kRowsThreads = 256;
constexpr int kRowsWaves = kRowsThreads / 64;
constexpr int kRowsLoads = 4;
static_assert(kRowsChunk == kRowsThreads * kRowsLoads * 2,
              "a chunk is four 16-B loads of two labels per thread");
constexpr int kRowsChunkPairs = kRowsChunk / 2;
constexpr int kRowsScatterRows = 4;

// Labels 2v and 2v + 1; a label past the end reads as `ignore`.  Only a pair
// that lies inside the array is read as one 16-B load.
__device__ __forceinline__ void rows_load2(const long long* __restrict__ labels,
                                           long long M, long long v,
                                           long long ignore,
                                           long long (&l)[2]) {
  if (2 * v + 1 < M) {
    const ulonglong2 q = ((const ulonglong2*)labels)[v];
    l[0] = (long long)q.x;
    l[1] = (long long)q.y;
  } else {
    l[0] = 2 * v < M ? labels[2 * v] : ignore;
    l[1] = ignore;
  }
}

// Sum of v over the block, in every thread, which all have to call it.
__device__ __forceinline__ int rows_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kRowsWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

// This thread's share of the labelled rows of chunk c.
__device__ __forceinline__ int rows_chunk_part(
    const long long* __restrict__ labels, long long M, long long c,
    long long ignore) {
  long long l[kRowsLoads][2];
#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j)
    rows_load2(labels, M, c * kRowsChunkPairs + j * kRowsThreads + threadIdx.x,
               ignore, l[j]);
  int n = 0;
#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j)
    n += (int)(l[j][0] != ignore) + (int)(l[j][1] != ignore);
  return n;
}

// counts[c] = the labelled rows of chunk c = blockIdx.x.
__global__ __launch_bounds__(kRowsThreads) void rows_count_k(
    const long long* __restrict__ labels, long long M, long long ignore,
    int* __restrict__ counts) {
  __shared__ int red[kRowsWaves];
  const int n =
      rows_block_sum(rows_chunk_part(labels, M, blockIdx.x, ignore), red);
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

template <bool COUNTS>
__global__ __launch_bounds__(kRowsThreads) void rows_index_k(
    const long long* __restrict__ labels, long long M, long long ignore,
    const int* __restrict__ counts, int* __restrict__ idx,
    int* __restrict__ rank, long long* __restrict__ row_labels,
    int* __restrict__ count, int capacity) {
  __shared__ int red[kRowsWaves];
  __shared__ int seg[kRowsLoads * kRowsWaves];
  const int chunk = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  int part = 0;
  if (COUNTS) {
    for (int c = threadIdx.x; c < chunk; c += kRowsThreads) part += counts[c];
  } else {
    // every chunk before this one is a whole one
#pragma unroll 2
    for (int c = 0; c < chunk; ++c)
      part += rows_chunk_part(labels, M, c, ignore);
  }
  const int base = rows_block_sum(part, red);

  const long long v0 = (long long)chunk * kRowsChunkPairs + threadIdx.x;
  long long l[kRowsLoads][2];
#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j)
    rows_load2(labels, M, v0 + j * kRowsThreads, ignore, l[j]);
  // labelled rows of segment (j, wave) before this lane's pair
  int before[kRowsLoads];
  const unsigned long long below = (1ULL << lane) - 1ULL;
#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j) {
    const unsigned long long b0 = __ballot(l[j][0] != ignore);
    const unsigned long long b1 = __ballot(l[j][1] != ignore);
    before[j] = __popcll(b0 & below) + __popcll(b1 & below);
    if (lane == 0) seg[j * kRowsWaves + wave] = __popcll(b0) + __popcll(b1);
  }
  __syncthreads();
  int r = base;
  int first[kRowsLoads];
#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j) {
#pragma unroll
    for (int w = 0; w < kRowsWaves; ++w) {
      if (w == wave) first[j] = r + before[j];
      r += seg[j * kRowsWaves + w];
    }
  }
  // r: the labelled rows up to the end of this chunk

#pragma unroll
  for (int j = 0; j < kRowsLoads; ++j) {
    const long long p = 2 * (v0 + j * kRowsThreads);
    const bool f0 = l[j][0] != ignore, f1 = l[j][1] != ignore;
    const int r0 = first[j], r1 = first[j] + (int)f0;
    if (p + 1 < M)
      ((int2*)rank)[p / 2] = make_int2(f0 ? r0 : -1, f1 ? r1 : -1);
    else if (p < M)
      rank[p] = f0 ? r0 : -1;
    // a label past M reads as ignore, so f0 means p < M and f1 p + 1 < M
    if (f0 && r0 < capacity) {
      idx[r0] = (int)p;
      row_labels[r0] = l[j][0];
    }
    if (f1 && r1 < capacity) {
      idx[r1] = (int)(p + 1);
      row_labels[r1] = l[j][1];
    }
  }
  if (chunk == (int)gridDim.x - 1) {
    if (threadIdx.x == 0) count[0] = r;
    for (long long t = (long long)r + threadIdx.x; t < capacity;
         t += kRowsThreads) {
      idx[t] = -1;
      row_labels[t] = ignore;
    }
  }
}

// One wave per block; vpr 16-B vectors per row.
__global__ __launch_bounds__(64) void rows_gather_k(
    const uint4* __restrict__ x, const int* __restrict__ idx,
    const int* __restrict__ count, uint4* __restrict__ rows, long long M,
    int capacity, int vpr, unsigned int nan_word) {
  const int n = count[0];
  const long long r0 = (long long)blockIdx.x * kRowsGatherRows;
  // the source row, or -1 for a row that is all `fill` words
  int src[kRowsGatherRows];
  unsigned int fill[kRowsGatherRows];
#pragma unroll
  for (int j = 0; j < kRowsGatherRows; ++j) {
    src[j] = -1;
    fill[j] = 0u;
    if (n > capacity) {
      fill[j] = nan_word;
    } else if (r0 + j < n) {
      const int p = idx[r0 + j];
      if (p >= 0 && p < M) src[j] = p; else fill[j] = nan_word;
    }
  }
#pragma unroll 2
  for (int v = threadIdx.x; v < vpr; v += 64) {
    uint4 q[kRowsGatherRows];
#pragma unroll
    for (int j = 0; j < kRowsGatherRows; ++j) {
      q[j] = make_uint4(fill[j], fill[j], fill[j], fill[j]);
      if (src[j] >= 0) q[j] = x[(size_t)src[j] * vpr + v];
    }
#pragma unroll
    for (int j = 0; j < kRowsGatherRows; ++j)
      if (r0 + j < capacity) rows[(size_t)(r0 + j) * vpr + v] = q[j];
  }
}

// The grid's threads are a multiple of vpr (grid_for), so a thread keeps its
// column vector and steps `step` rows.
__global__ __launch_bounds__(kRowsThreads) void rows_scatter_k(
    const uint4* __restrict__ d_rows, const int* __restrict__ rank,
    uint4* __restrict__ dx, long long M, int capacity, int vpr) {
  const long long t = (long long)blockIdx.x * kRowsThreads + threadIdx.x;
  const long long step = (long long)gridDim.x * kRowsThreads / vpr;
  const int c = (int)(t % vpr);
  for (long long row = t / vpr; row < M; row += step * kRowsScatterRows) {
    int k[kRowsScatterRows];
    uint4 q[kRowsScatterRows];
#pragma unroll
    for (int j = 0; j < kRowsScatterRows; ++j) {
      const long long rr = row + j * step;
      k[j] = rr < M ? rank[rr] : -1;
    }
#pragma unroll
    for (int j = 0; j < kRowsScatterRows; ++j) {
      q[j] = make_uint4(0u, 0u, 0u, 0u);
      if (k[j] >= 0 && k[j] < capacity) q[j] = d_rows[(size_t)k[j] * vpr + c];
    }
#pragma unroll
    for (int j = 0; j < kRowsScatterRows; ++j) {
      const long long rr = row + j * step;
      if (rr < M) dx[(size_t)rr * vpr + c] = q[j];
    }
  }
}

bool rows_shape_ok(long long M, long long capacity, long long row_bytes) {
  return M >= 1 && M <= kRowsMaxM && capacity >= 1 && capacity <= kRowsMaxM &&
         row_bytes >= 16 && row_bytes <= kRowsMaxRowBytes &&
         row_bytes % 16 == 0;
}

}  // namespace

int RowsIndexChunks(long long M) {
  return (int)((M + kRowsChunk - 1) / kRowsChunk);
}

bool RowsIndexUsesCounts(long long M) {
  return RowsIndexChunks(M) > kRowsRecountMaxChunks;
}

hipError_t RowsIndexLaunch(const long long* labels, long long M,
                           long long ignore_index, long long capacity,
                           int* counts, int* idx, int* rank,
                           long long* row_labels, int* count,
                           hipStream_t stream) {
  const void* p16[] = {labels, row_labels};
  const void* p8[] = {rank};
  if (!labels || !idx || !rank || !row_labels || !count ||
      !rows_shape_ok(M, capacity, 16) || !aligned_to(p16, 2, 16) ||
      !aligned_to(p8, 1, 8))
    return hipErrorInvalidValue;
  const int chunks = RowsIndexChunks(M);
  if (counts) {
    rows_count_k<<<chunks, kRowsThreads, 0, stream>>>(labels, M, ignore_index,
                                                      counts);
    rows_index_k<true><<<chunks, kRowsThreads, 0, stream>>>(
        labels, M, ignore_index, counts, idx, rank, row_labels, count,
        (int)capacity);
  } else {
    rows_index_k<false><<<chunks, kRowsThreads, 0, stream>>>(
        labels, M, ignore_index, nullptr, idx, rank, row_labels, count,
        (int)capacity);
  }
  return hipGetLastError();
}

hipError_t RowsGatherLaunch(const void* x, const int* idx, const int* count,
                            void* rows, long long M, long long capacity,
                            long long row_bytes, int dt, hipStream_t stream) {
  const void* ptrs[] = {x, rows};
  if (!x || !idx || !count || !rows || !rows_shape_ok(M, capacity, row_bytes) ||
      !aligned_to(ptrs, 2, 16))
    return hipErrorInvalidValue;
  unsigned int nan_word;
  switch (dt) {
    case DT_F32: nan_word = 0x7FC00000u; break;
    case DT_F16: nan_word = 0x7E007E00u; break;
    case DT_BF16: nan_word = 0x7FC07FC0u; break;
    default: return hipErrorInvalidValue;
  }
  const long long blocks = (capacity + kRowsGatherRows - 1) / kRowsGatherRows;
  rows_gather_k<<<(unsigned)blocks, 64, 0, stream>>>(
      (const uint4*)x, idx, count, (uint4*)rows, M, (int)capacity,
      (int)(row_bytes / 16), nan_word);
  return hipGetLastError();
}

hipError_t RowsScatterLaunch(const void* d_rows, const int* rank, void* dx,
                             long long M, long long capacity,
                             long long row_bytes, hipStream_t stream) {
  const void* ptrs[] = {d_rows, dx};
  if (!d_rows || !rank || !dx || !rows_shape_ok(M, capacity, row_bytes) ||
      !aligned_to(ptrs, 2, 16))
    return hipErrorInvalidValue;
  const int vpr = (int)(row_bytes / 16);
  // grid_for speaks of 8-element vectors of rows of C elements
  const int blocks = grid_for(M * vpr * 8, vpr * 8);
  rows_scatter_k<<<blocks, kRowsThreads, 0, stream>>>(
      (const uint4*)d_rows, rank, (uint4*)dx, M, (int)capacity, vpr);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
