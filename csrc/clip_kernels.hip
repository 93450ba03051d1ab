// Global-norm gradient clipping for CDNA4: a multi-tensor squared-norm pass,
// a one-block finalize that turns the block partials into {total_norm, coef},
// and an in-place multi-tensor scale that reads coef from device memory.  A
// second finalize serves loss scaling: it also unscales, flags an overflow
// and updates the scale on the device (scaled_clip_finalize_k).
//
// Work is divided by elements, not by tensor: every block owns one fixed
// kChunkElems-element chunk of one tensor and finds its tensor by searching
// the per-tensor block prefix in the kernel args, so a 31 M-element embedding
// gets ~3800 blocks and a 1024-element bias gets one.
//
// Determinism: each block writes its partial to its own workspace slot and
// the finalize kernel sums the slots in a fixed order (fp64).  There are no
// atomics, so identical inputs give bitwise identical {norm, coef} — every
// data-parallel rank must clip by exactly the same coefficient.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

constexpr int kFinalizeThreads = 1024;

template <typename T>
__global__ __launch_bounds__(kChunkThreads) void multi_sqnorm_k(
    ClipBatchArgs args, float* __restrict__ partials) {
  const ChunkRef c = find_chunk(args);
  const T* __restrict__ p = (const T*)args.ptr[0][c.tensor];
  constexpr int VS = 16 / (int)sizeof(T);

  // independent accumulators keep several 16-byte loads in flight
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  long long done = c.begin;
  // chunk starts are multiples of kChunkElems elements, so the chunk is
  // 16-byte aligned exactly when the tensor is
  if (((uintptr_t)p & 15) == 0) {
    const long long nvec = (c.end - c.begin) / VS;
    const uint4* __restrict__ pv = (const uint4*)(p + c.begin);
    done = c.begin + nvec * VS;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      union {
        uint4 u;
        T e[VS];
      } in;
      in.u = pv[i];
#pragma unroll
      for (int v = 0; v < VS; ++v) {
        float f = (float)in.e[v];
        acc[v & 3] += f * f;
      }
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    float f = (float)p[i];
    acc[0] += f * f;
  }
  const float total = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) partials[args.partial_base + blockIdx.x] = total;
}

// One block: thread t sums slots t, t + 1024, ... in fp64, then a fixed LDS
// tree.  out[0] = total_norm, out[1] = clip coefficient, following
// torch.nn.utils.clip_grad_norm_: reciprocal(total_norm + 1e-6) * max_norm
// in fp32, clamped to at most 1.  The clamp is a compare, not fminf, so a
// NaN norm stays a NaN coefficient; an infinite norm gives 0.
__global__ __launch_bounds__(kFinalizeThreads) void clip_finalize_k(
    const float* __restrict__ partials, long long n, float max_norm,
    float* __restrict__ out) {
  __shared__ double part[kFinalizeThreads];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kFinalizeThreads)
    s += (double)partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int half = kFinalizeThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total_norm = (float)sqrt(part[0]);
    float coef = (1.0f / (total_norm + 1e-6f)) * max_norm;
    if (coef > 1.0f) coef = 1.0f;
    out[0] = total_norm;
    out[1] = coef;
  }
}

// clip_finalize_k for a loss-scaled step (ScaledFinalizeParams, kernels.h):
// the same sum in the same order, then {total_norm, coef, found, S} and the
// scale update, all by thread 0.  A non-finite sum of squares is the overflow
// test: every inf or NaN element makes it so, and so do finite gradients
// whose norm passes sqrt(FLT_MAX) ~ 1.8e19 -- for a loss scaler also "scale
// too high".  The scale is read before it is updated: out[3] and coef belong
// to the gradients at hand.
__global__ __launch_bounds__(kFinalizeThreads) void scaled_clip_finalize_k(
    const float* __restrict__ partials, long long n, ScaledFinalizeParams p,
    float* __restrict__ out) {
  __shared__ double part[kFinalizeThreads];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kFinalizeThreads)
    s += (double)partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int half = kFinalizeThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double sum = part[0];
  const float scale = p.scale ? *p.scale : 1.0f;
  // x - x is 0 for finite x and NaN for inf and NaN
  bool found = !(sum - sum == 0.0);
  if (p.found_inf && *p.found_inf != 0.0f) found = true;
  const float inv = 1.0f / scale;
  const float total_norm = (float)sqrt(sum) * inv;
  float clip = 1.0f;
  if (p.has_max_norm) {
    clip = (1.0f / (total_norm + 1e-6f)) * p.max_norm;
    if (clip > 1.0f) clip = 1.0f;  // a compare: NaN stays NaN
  }
  out[0] = total_norm;
  out[1] = clip * inv;
  out[2] = found ? 1.0f : 0.0f;
  out[3] = scale;
  if (!p.growth_tracker) return;
  if (found) {
    *p.scale = scale * p.backoff_factor;
    *p.growth_tracker = 0;
    return;
  }
  const int successive = *p.growth_tracker + 1;
  if (successive == p.growth_interval) {
    const float grown = scale * p.growth_factor;
    if (grown - grown == 0.0f) *p.scale = grown;
    *p.growth_tracker = 0;
  } else {
    *p.growth_tracker = successive;
  }
}

template <typename T>
__global__ __launch_bounds__(kChunkThreads) void multi_scale_k(
    ClipBatchArgs args, const float* __restrict__ coef_ptr) {
  const float coef = *coef_ptr;
  // nothing to clip: leave memory untouched (NaN compares unequal and
  // falls through, so a NaN norm still poisons the gradients like torch)
  if (coef == 1.0f) return;
  const ChunkRef c = find_chunk(args);
  T* __restrict__ p = (T*)args.ptr[0][c.tensor];
  constexpr int VS = 16 / (int)sizeof(T);

  long long done = c.begin;
  if (((uintptr_t)p & 15) == 0) {
    const long long nvec = (c.end - c.begin) / VS;
    uint4* __restrict__ pv = (uint4*)(p + c.begin);
    done = c.begin + nvec * VS;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      union {
        uint4 u;
        T e[VS];
      } io;
      io.u = pv[i];
#pragma unroll
      for (int v = 0; v < VS; ++v) io.e[v] = (T)((float)io.e[v] * coef);
      pv[i] = io.u;
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads)
    p[i] = (T)((float)p[i] * coef);
}

}  // namespace

hipError_t MultiSqNormLaunch(const ClipBatchArgs& args, int dt,
                             float* partials, hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  switch (dt) {
    case DT_F32:
      multi_sqnorm_k<float><<<grid, block, 0, stream>>>(args, partials);
      break;
    case DT_F16:
      multi_sqnorm_k<__half><<<grid, block, 0, stream>>>(args, partials);
      break;
    case DT_BF16:
      multi_sqnorm_k<__hip_bfloat16><<<grid, block, 0, stream>>>(args,
                                                                 partials);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t ClipFinalizeLaunch(const float* partials, long long n_partials,
                              float max_norm, float* out,
                              hipStream_t stream) {
  clip_finalize_k<<<dim3(1), dim3(kFinalizeThreads), 0, stream>>>(
      partials, n_partials, max_norm, out);
  return hipGetLastError();
}

hipError_t ScaledClipFinalizeLaunch(const float* partials,
                                    long long n_partials,
                                    const ScaledFinalizeParams& p, float* out,
                                    hipStream_t stream) {
  if (p.growth_tracker && !p.scale) return hipErrorInvalidValue;
  scaled_clip_finalize_k<<<dim3(1), dim3(kFinalizeThreads), 0, stream>>>(
      partials, n_partials, p, out);
  return hipGetLastError();
}

hipError_t MultiScaleLaunch(const ClipBatchArgs& args, int dt,
                            const float* coef, hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  switch (dt) {
    case DT_F32:
      multi_scale_k<float><<<grid, block, 0, stream>>>(args, coef);
      break;
    case DT_F16:
      multi_scale_k<__half><<<grid, block, 0, stream>>>(args, coef);
      break;
    case DT_BF16:
      multi_scale_k<__hip_bfloat16><<<grid, block, 0, stream>>>(args, coef);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
