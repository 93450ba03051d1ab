// Fused LAMB step for CDNA4: per batch of at most kCopyBatchCapacity fp32
// tensors, three launches replace ~15 eager kernels and two norm launches
// per parameter.
//
//   1. lamb_moments_k   m, v updated in place; u = mhat / (sqrt(vhat) + eps)
//                       + weight_decay * p formed in registers; the block's
//                       sum(p^2) and sum(u^2) go to its own workspace slots
//   2. lamb_trust_k     one block per tensor sums that tensor's slots in
//                       fp64 and writes the trust ratio |p| / |u|
//   3. lamb_update_k    p -= lr * trust * u, u recomputed from the updated
//                       moments (10 fp32 accesses per element either way,
//                       and no model-sized temporary)
//
// Work is divided like the clip kernels: every block of 1. and 3. owns one
// kChunkElems-element chunk of one tensor (multi_tensor.h).  There are no
// atomics and every sum runs in a fixed order, so identical inputs give
// bitwise identical trust ratios: data-parallel ranks hold replicated
// parameters and averaged gradients and must derive the same ratios without
// a collective.
//
// Bias correction is folded on the host into inv_bc1 and inv_bc2_sqrt, so
// the per-element body is one sqrtf, one divide and FMAs.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

constexpr int kTrustThreads = 256;

template <bool HAS_COEF>
__global__ __launch_bounds__(kChunkThreads) void lamb_moments_k(
    LambBatchArgs args, LambScalars s, const float* __restrict__ grad_coef,
    float* __restrict__ partials) {
  const ChunkRef c = find_chunk(args);
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  const float* __restrict__ p = (const float*)args.ptr[kRowParam][c.tensor];
  const float* __restrict__ g = (const float*)args.ptr[kRowGrad][c.tensor];
  float* __restrict__ m = (float*)args.ptr[kRowExpAvg][c.tensor];
  float* __restrict__ v = (float*)args.ptr[kRowExpAvgSq][c.tensor];

  // independent accumulators, one per lane of the 16-byte vector
  float pp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float uu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  long long done = c.begin;
  // chunk starts are multiples of kChunkElems elements, so the chunk is
  // 16-byte aligned exactly when the tensor is
  if (aligned16(p, g, m, v)) {
    const long long nvec = (c.end - c.begin) / 4;
    const float4* __restrict__ p4 = (const float4*)(p + c.begin);
    const float4* __restrict__ g4 = (const float4*)(g + c.begin);
    float4* __restrict__ m4 = (float4*)(m + c.begin);
    float4* __restrict__ v4 = (float4*)(v + c.begin);
    done = c.begin + nvec * 4;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      const float4 pv = p4[i];
      const float4 gv = g4[i];
      float4 mv = m4[i];
      float4 vv = v4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lamb_moments_element<HAS_COEF>((&pv.x)[k], (&gv.x)[k], (&mv.x)[k],
                                       (&vv.x)[k], coef, s, pp[k], uu[k]);
      m4[i] = mv;
      v4[i] = vv;
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    lamb_moments_element<HAS_COEF>(p[i], g[i], m[i], v[i], coef, s, pp[0],
                                   uu[0]);
  }
  const float pp_total = block_sum((pp[0] + pp[1]) + (pp[2] + pp[3]));
  // block_sum's LDS is shared by both calls: thread 0 must be done reading
  __syncthreads();
  const float uu_total = block_sum((uu[0] + uu[1]) + (uu[2] + uu[3]));
  if (threadIdx.x == 0) {
    float* slot = partials + 2 * (args.partial_base + blockIdx.x);
    slot[0] = pp_total;
    slot[1] = uu_total;
  }
}

// Block t handles tensor t of the batch: thread i sums the slot pairs i,
// i + 256, ... of the tensor in fp64 (a 31 M-element embedding has ~3800),
// then a fixed LDS tree.
__global__ __launch_bounds__(kTrustThreads) void lamb_trust_k(
    LambBatchArgs args, const float* __restrict__ partials, bool adapt,
    float* __restrict__ trust) {
  __shared__ double part_p[kTrustThreads];
  __shared__ double part_u[kTrustThreads];
  const int t = blockIdx.x;
  const unsigned int first = args.block_prefix[t];
  const unsigned int n = args.block_prefix[t + 1] - first;
  const float* __restrict__ slots = partials + 2 * (args.partial_base + first);
  double sp = 0.0, su = 0.0;
  for (unsigned int i = threadIdx.x; i < n; i += kTrustThreads) {
    sp += (double)slots[2 * (unsigned long long)i];
    su += (double)slots[2 * (unsigned long long)i + 1];
  }
  part_p[threadIdx.x] = sp;
  part_u[threadIdx.x] = su;
  __syncthreads();
  for (int half = kTrustThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      part_p[threadIdx.x] += part_p[threadIdx.x + half];
      part_u[threadIdx.x] += part_u[threadIdx.x + half];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double w_norm = sqrt(part_p[0]);
    const double u_norm = sqrt(part_u[0]);
    // compares, so a NaN norm gives trust 1
    float r = 1.0f;
    if (adapt && w_norm > 0.0 && u_norm > 0.0) r = (float)(w_norm / u_norm);
    trust[args.out_index[t]] = r;
  }
}

__global__ __launch_bounds__(kChunkThreads) void lamb_update_k(
    LambBatchArgs args, LambScalars s, const float* __restrict__ trust) {
  const ChunkRef c = find_chunk(args);
  const float step = s.lr * trust[args.out_index[c.tensor]];
  float* __restrict__ p = (float*)args.ptr[kRowParam][c.tensor];
  const float* __restrict__ m = (const float*)args.ptr[kRowExpAvg][c.tensor];
  const float* __restrict__ v = (const float*)args.ptr[kRowExpAvgSq][c.tensor];

  long long done = c.begin;
  if (aligned16(p, m, v)) {
    const long long nvec = (c.end - c.begin) / 4;
    float4* __restrict__ p4 = (float4*)(p + c.begin);
    const float4* __restrict__ m4 = (const float4*)(m + c.begin);
    const float4* __restrict__ v4 = (const float4*)(v + c.begin);
    done = c.begin + nvec * 4;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      float4 pv = p4[i];
      const float4 mv = m4[i];
      const float4 vv = v4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lamb_update_element((&pv.x)[k], (&mv.x)[k], (&vv.x)[k], step, s);
      p4[i] = pv;
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    float pe = p[i];
    lamb_update_element(pe, m[i], v[i], step, s);
    p[i] = pe;
  }
}

}  // namespace

LambScalars LambFoldScalars(float lr, float beta1, float beta2, float eps,
                            float weight_decay, long long step,
                            bool bias_correction) {
  LambScalars s;
  s.lr = lr;
  s.beta1 = beta1;
  s.beta2 = beta2;
  s.eps = eps;
  s.weight_decay = weight_decay;
  s.inv_bc1 = 1.0f;
  s.inv_bc2_sqrt = 1.0f;
  if (bias_correction) {
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    s.inv_bc1 = (float)(1.0 / bc1);
    s.inv_bc2_sqrt = (float)(1.0 / std::sqrt(bc2));
  }
  return s;
}

hipError_t LambMomentsLaunch(const LambBatchArgs& args, const LambScalars& s,
                             const float* grad_coef, float* partials,
                             hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  auto kernel = grad_coef ? lamb_moments_k<true> : lamb_moments_k<false>;
  kernel<<<grid, block, 0, stream>>>(args, s, grad_coef, partials);
  return hipGetLastError();
}

hipError_t LambTrustLaunch(const LambBatchArgs& args, const float* partials,
                           bool adapt, float* trust, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  lamb_trust_k<<<dim3(args.count), dim3(kTrustThreads), 0, stream>>>(
      args, partials, adapt, trust);
  return hipGetLastError();
}

hipError_t LambUpdateLaunch(const LambBatchArgs& args, const LambScalars& s,
                            const float* trust, hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  lamb_update_k<<<grid, block, 0, stream>>>(args, s, trust);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace hvd
