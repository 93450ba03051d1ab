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
//
// Master weights (LP, multi_tensor.h): p is the fp32 master, 1. reads a
// 2-byte gradient, norms and trust ratios are the master's, and 3. also
// writes the rounded master into the 2-byte model parameter.  The bytes
// moved stay 40 per element (22 + 18 instead of 24 + 16).
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

constexpr int kTrustThreads = 256;

template <typename LP>
using LambArgsOf = typename std::conditional<LowPrec<LP>::kModel,
                                             LambMasterBatchArgs,
                                             LambBatchArgs>::type;

// LP: void, or the 2-byte type of the gradient and the model parameter
// (master weights, multi_tensor.h); p is then the fp32 master.
template <typename LP, bool HAS_COEF>
__global__ __launch_bounds__(kChunkThreads) void lamb_moments_k(
    LambArgsOf<LP> args, LambScalars s, const float* __restrict__ grad_coef,
    const float* __restrict__ skip, float* __restrict__ partials) {
  using G = typename LowPrec<LP>::Grad;
  constexpr int W = LowPrec<LP>::kVec;
  // one uniform load: a set flag (an overflowed step) leaves the moments as
  // they are and the partials unwritten (lamb_trust_k does not read them)
  if (skip && *skip != 0.0f) return;
  const ChunkRef c = find_chunk(args);
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  const float* __restrict__ p = (const float*)args.ptr[kRowParam][c.tensor];
  const G* __restrict__ g = (const G*)args.ptr[kRowGrad][c.tensor];
  float* __restrict__ m = (float*)args.ptr[kRowExpAvg][c.tensor];
  float* __restrict__ v = (float*)args.ptr[kRowExpAvgSq][c.tensor];

  // independent accumulators, one per lane of a 16-byte fp32 vector
  float pp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float uu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  long long done = c.begin;
  // chunk starts are multiples of kChunkElems elements, so the chunk is
  // 16-byte aligned exactly when the tensor is
  if (aligned16(p, g, m, v)) {
    const long long nvec = (c.end - c.begin) / W;
    done = c.begin + nvec * W;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      float pv[W], gv[W], mv[W], vv[W];
      load_f32_vec(p + c.begin, i, pv);
      load_grad_vec(g + c.begin, i, gv);
      load_f32_vec(m + c.begin, i, mv);
      load_f32_vec(v + c.begin, i, vv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        lamb_moments_element<HAS_COEF>(pv[k], gv[k], mv[k], vv[k], coef, s,
                                       pp[k & 3], uu[k & 3]);
      store_f32_vec(m + c.begin, i, mv);
      store_f32_vec(v + c.begin, i, vv);
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    lamb_moments_element<HAS_COEF>(p[i], (float)g[i], m[i], v[i], coef, s,
                                   pp[0], uu[0]);
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
// then a fixed LDS tree.  Args: LambBatchArgs or LambMasterBatchArgs.
template <typename Args>
__global__ __launch_bounds__(kTrustThreads) void lamb_trust_k(
    Args args, const float* __restrict__ partials, bool adapt,
    const float* __restrict__ skip, float* __restrict__ trust) {
  __shared__ double part_p[kTrustThreads];
  __shared__ double part_u[kTrustThreads];
  const int t = blockIdx.x;
  // a skipped step wrote no partials: the ratio is defined as 1
  if (skip && *skip != 0.0f) {
    if (threadIdx.x == 0) trust[args.out_index[t]] = 1.0f;
    return;
  }
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

// With LP the updated master also goes to the model parameter, rounded.
template <typename LP>
__global__ __launch_bounds__(kChunkThreads) void lamb_update_k(
    LambArgsOf<LP> args, LambScalars s, const float* __restrict__ trust,
    const float* __restrict__ skip) {
  using Q = typename LowPrec<LP>::Grad;
  constexpr bool MODEL = LowPrec<LP>::kModel;
  constexpr int W = LowPrec<LP>::kVec;
  if (skip && *skip != 0.0f) return;  // as lamb_moments_k
  const ChunkRef c = find_chunk(args);
  const float step = s.lr * trust[args.out_index[c.tensor]];
  float* __restrict__ p = (float*)args.ptr[kRowParam][c.tensor];
  const float* __restrict__ m = (const float*)args.ptr[kRowExpAvg][c.tensor];
  const float* __restrict__ v = (const float*)args.ptr[kRowExpAvgSq][c.tensor];
  Q* __restrict__ q = nullptr;  // stays null without a model row
  if constexpr (MODEL) q = (Q*)args.ptr[kRowModel][c.tensor];

  long long done = c.begin;
  if (aligned16(p, m, v, q)) {
    const long long nvec = (c.end - c.begin) / W;
    done = c.begin + nvec * W;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      float pv[W], mv[W], vv[W];
      load_f32_vec(p + c.begin, i, pv);
      load_f32_vec(m + c.begin, i, mv);
      load_f32_vec(v + c.begin, i, vv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        lamb_update_element(pv[k], mv[k], vv[k], step, s);
      store_f32_vec(p + c.begin, i, pv);
      if constexpr (MODEL) store_lp_vec(q + c.begin, i, pv);
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    float pe = p[i];
    lamb_update_element(pe, m[i], v[i], step, s);
    p[i] = pe;
    if constexpr (MODEL) q[i] = round_lp<Q>(pe);
  }
}

template <typename LP>
hipError_t launch_moments(const LambArgsOf<LP>& args, const LambScalars& s,
                          const float* grad_coef, const float* skip,
                          float* partials, hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  auto kernel =
      grad_coef ? lamb_moments_k<LP, true> : lamb_moments_k<LP, false>;
  kernel<<<grid, block, 0, stream>>>(args, s, grad_coef, skip, partials);
  return hipGetLastError();
}

template <typename Args>
hipError_t launch_trust(const Args& args, const float* partials, bool adapt,
                        const float* skip, float* trust, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  lamb_trust_k<Args><<<dim3(args.count), dim3(kTrustThreads), 0, stream>>>(
      args, partials, adapt, skip, trust);
  return hipGetLastError();
}

template <typename LP>
hipError_t launch_update(const LambArgsOf<LP>& args, const LambScalars& s,
                         const float* trust, const float* skip,
                         hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  lamb_update_k<LP><<<grid, block, 0, stream>>>(args, s, trust, skip);
  return hipGetLastError();
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
                             const float* grad_coef, const float* skip,
                             float* partials, hipStream_t stream) {
  return launch_moments<void>(args, s, grad_coef, skip, partials, stream);
}

hipError_t LambTrustLaunch(const LambBatchArgs& args, const float* partials,
                           bool adapt, const float* skip, float* trust,
                           hipStream_t stream) {
  return launch_trust(args, partials, adapt, skip, trust, stream);
}

hipError_t LambUpdateLaunch(const LambBatchArgs& args, const LambScalars& s,
                            const float* trust, const float* skip,
                            hipStream_t stream) {
  return launch_update<void>(args, s, trust, skip, stream);
}

hipError_t LambMomentsMasterLaunch(const LambMasterBatchArgs& args, int dt,
                                   const LambScalars& s,
                                   const float* grad_coef, const float* skip,
                                   float* partials, hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_moments<__half>(args, s, grad_coef, skip, partials,
                                    stream);
    case DT_BF16:
      return launch_moments<__hip_bfloat16>(args, s, grad_coef, skip,
                                            partials, stream);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t LambTrustLaunch(const LambMasterBatchArgs& args,
                           const float* partials, bool adapt,
                           const float* skip, float* trust,
                           hipStream_t stream) {
  return launch_trust(args, partials, adapt, skip, trust, stream);
}

hipError_t LambUpdateMasterLaunch(const LambMasterBatchArgs& args, int dt,
                                  const LambScalars& s, const float* trust,
                                  const float* skip, hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_update<__half>(args, s, trust, skip, stream);
    case DT_BF16:
      return launch_update<__hip_bfloat16>(args, s, trust, skip, stream);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace gpu
}  // namespace hvd
