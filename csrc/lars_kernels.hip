// Fused LARS step for CDNA4 (layer-wise adaptive rate scaling, You et al.
// 2017): momentum SGD whose step is scaled per tensor by a trust ratio.  Per
// batch of at most kCopyBatchCapacity tensors, three launches replace ~10
// eager kernels and two norm launches per parameter.
//
//   1. lars_norms_k    reads p and g; the block's sum(p^2) and sum(g'^2),
//                      g' = g * coef, go to its own workspace slots
//   2. lars_trust_k    one block per tensor sums that tensor's slots in fp64
//                      and writes the trust ratio
//                      trust_coefficient * |p| / (|g'| + weight_decay * |p|
//                      + eps)
//   3. lars_update_k   d = trust * (g' + weight_decay * p),
//                      m = momentum * m + d, p -= lr * (m, or d + momentum *
//                      m with nesterov)
//
// Work is divided like the clip and LAMB kernels: every block of 1. and 3.
// owns one kChunkElems-element chunk of one tensor (multi_tensor.h), so a
// ResNet's one large and many small tensors spread evenly, unlike under the
// fixed blocks-per-tensor grid of fused_sgd_k.  There are no atomics and every
// sum runs in a fixed order, so identical inputs give bitwise identical trust
// ratios: data-parallel ranks derive the same ratios without a collective.
//
// Bytes per element: 8 (norms) + 20 (update) = 28; fused_sgd_k moves 20.
//
// Master weights (LP, multi_tensor.h): p is the fp32 master, 1. reads a
// 2-byte gradient (6 bytes per element), norms and trust ratios are the
// master's, and 3. also writes the rounded master into the 2-byte model
// parameter (20 bytes: 4 + 2 + 4 read, 4 + 4 + 2 written).  Pass 1 sums in
// one order whatever the gradient's type and the alignment (see
// lars_norms_k), so such a step gives bitwise the master, momentum and trust
// ratios of the fp32 step on the widened gradient.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "multi_tensor.h"

namespace hvd {
namespace gpu {

namespace {

constexpr int kTrustThreads = 256;

template <typename LP>
using LarsArgsOf = typename std::conditional<LowPrec<LP>::kModel,
                                             LarsMasterBatchArgs,
                                             LarsBatchArgs>::type;

// 4 gradient elements in one load: 16 bytes of fp32, 8 bytes of a 2-byte type.
template <typename G>
__device__ __forceinline__ void load_grad_quad(const G* base, long long i,
                                               float (&x)[4]) {
  if constexpr (std::is_same<G, float>::value)
    load_f32_vec(base, i, x);
  else
    load_lp_quad(base, i, x);
}

// LP: void, or the 2-byte type of the gradient (master weights,
// multi_tensor.h); p is then the fp32 master.
//
// The chunk is walked in quads of 4 elements: lane i takes the quads i,
// i + 256, ... and adds element k of each to its accumulator k.  A whole
// quad of an aligned tensor is one 16-byte load of p and one 16- or 8-byte
// load of g; the ragged last quad, and every quad of a tensor that is not
// aligned, is read element by element into the same accumulators, so the
// sums do not depend on which way the data came in.
template <typename LP, bool HAS_COEF>
__global__ __launch_bounds__(kChunkThreads) void lars_norms_k(
    LarsArgsOf<LP> args, const float* __restrict__ grad_coef,
    const float* __restrict__ skip, float* __restrict__ partials) {
  using G = typename LowPrec<LP>::Grad;
  // one uniform load: a set flag (an overflowed step) leaves the partials
  // unwritten (lars_trust_k does not read them)
  if (skip && *skip != 0.0f) return;
  const ChunkRef c = find_chunk(args);
  // one uniform load; the gradient tensors are never written
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  const float* __restrict__ p =
      (const float*)args.ptr[kRowParam][c.tensor] + c.begin;
  const G* __restrict__ g = (const G*)args.ptr[kRowGrad][c.tensor] + c.begin;
  const long long len = c.end - c.begin;
  const long long nquad = (len + 3) / 4;
  // chunk starts are multiples of kChunkElems elements, so the chunk is
  // aligned exactly when the tensor is; a quad of g is 4 * sizeof(G) bytes
  const bool vec = aligned16(p) && ((uintptr_t)g & (4 * sizeof(G) - 1)) == 0;

  // independent accumulators, one per element of a quad
  float pp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float gg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (long long i = threadIdx.x; i < nquad; i += kChunkThreads) {
    if (vec && 4 * i + 4 <= len) {
      float pv[4], gv[4];
      load_f32_vec(p, i, pv);
      load_grad_quad(g, i, gv);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lars_norms_element<HAS_COEF>(pv[k], gv[k], coef, pp[k], gg[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long e = 4 * i + k;
        if (e < len)
          lars_norms_element<HAS_COEF>(p[e], (float)g[e], coef, pp[k], gg[k]);
      }
    }
  }
  const float pp_total = block_sum((pp[0] + pp[1]) + (pp[2] + pp[3]));
  // block_sum's LDS is shared by both calls: thread 0 must be done reading
  __syncthreads();
  const float gg_total = block_sum((gg[0] + gg[1]) + (gg[2] + gg[3]));
  if (threadIdx.x == 0) {
    float* slot = partials + 2 * (args.partial_base + blockIdx.x);
    slot[0] = pp_total;
    slot[1] = gg_total;
  }
}

// Block t handles tensor t of the batch: thread i sums the slot pairs i,
// i + 256, ... of the tensor in fp64, then a fixed LDS tree.  Args:
// LarsBatchArgs or LarsMasterBatchArgs.
template <typename Args>
__global__ __launch_bounds__(kTrustThreads) void lars_trust_k(
    Args args, LarsScalars s, const float* __restrict__ partials,
    const float* __restrict__ skip, float* __restrict__ trust) {
  __shared__ double part_p[kTrustThreads];
  __shared__ double part_g[kTrustThreads];
  const int t = blockIdx.x;
  // a skipped step wrote no partials: the ratio is defined as 1
  if (skip && *skip != 0.0f) {
    if (threadIdx.x == 0) trust[args.out_index[t]] = 1.0f;
    return;
  }
  const unsigned int first = args.block_prefix[t];
  const unsigned int n = args.block_prefix[t + 1] - first;
  const float* __restrict__ slots = partials + 2 * (args.partial_base + first);
  double sp = 0.0, sg = 0.0;
  for (unsigned int i = threadIdx.x; i < n; i += kTrustThreads) {
    sp += (double)slots[2 * (unsigned long long)i];
    sg += (double)slots[2 * (unsigned long long)i + 1];
  }
  part_p[threadIdx.x] = sp;
  part_g[threadIdx.x] = sg;
  __syncthreads();
  for (int half = kTrustThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      part_p[threadIdx.x] += part_p[threadIdx.x + half];
      part_g[threadIdx.x] += part_g[threadIdx.x + half];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double w_norm = sqrt(part_p[0]);
    const double g_norm = sqrt(part_g[0]);
    // compares, so a NaN norm gives trust 1
    float r = 1.0f;
    if (s.adapt && w_norm > 0.0 && g_norm > 0.0) {
      r = (float)((double)s.trust_coefficient * w_norm /
                  (g_norm + (double)s.weight_decay * w_norm + (double)s.eps));
      if (s.trust_clip) {
        // fp32: lr == 0 gives inf (or NaN from 0 / 0), hence 1
        const float clipped = r / s.lr;
        r = clipped < 1.0f ? clipped : 1.0f;
      }
    }
    trust[args.out_index[t]] = r;
  }
}

// With LP the gradient is 2-byte and the updated master also goes to the
// model parameter, rounded.
template <typename LP, bool NESTEROV, bool HAS_COEF>
__global__ __launch_bounds__(kChunkThreads) void lars_update_k(
    LarsArgsOf<LP> args, LarsScalars s, const float* __restrict__ grad_coef,
    const float* __restrict__ trust, const float* __restrict__ skip) {
  using G = typename LowPrec<LP>::Grad;
  constexpr bool MODEL = LowPrec<LP>::kModel;
  constexpr int W = LowPrec<LP>::kVec;
  if (skip && *skip != 0.0f) return;  // as lars_norms_k
  const ChunkRef c = find_chunk(args);
  const float coef = HAS_COEF ? *grad_coef : 1.0f;
  const float r = trust[args.out_index[c.tensor]];
  float* __restrict__ p = (float*)args.ptr[kRowParam][c.tensor];
  const G* __restrict__ g = (const G*)args.ptr[kRowGrad][c.tensor];
  float* __restrict__ m = (float*)args.ptr[kRowMomentum][c.tensor];
  G* __restrict__ q = nullptr;  // stays null without a model row
  if constexpr (MODEL) q = (G*)args.ptr[kRowSgdModel][c.tensor];

  long long done = c.begin;
  if (aligned16(p, g, m, q)) {
    const long long nvec = (c.end - c.begin) / W;
    done = c.begin + nvec * W;
    for (long long i = threadIdx.x; i < nvec; i += kChunkThreads) {
      float pv[W], gv[W], mv[W];
      load_f32_vec(p + c.begin, i, pv);
      load_grad_vec(g + c.begin, i, gv);
      load_f32_vec(m + c.begin, i, mv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        lars_element<NESTEROV, HAS_COEF>(pv[k], gv[k], mv[k], coef, r, s.lr,
                                         s.momentum, s.weight_decay);
      store_f32_vec(p + c.begin, i, pv);
      store_f32_vec(m + c.begin, i, mv);
      if constexpr (MODEL) store_lp_vec(q + c.begin, i, pv);
    }
  }
  for (long long i = done + threadIdx.x; i < c.end; i += kChunkThreads) {
    float pe = p[i], me = m[i];
    lars_element<NESTEROV, HAS_COEF>(pe, (float)g[i], me, coef, r, s.lr,
                                     s.momentum, s.weight_decay);
    p[i] = pe;
    m[i] = me;
    if constexpr (MODEL) q[i] = round_lp<G>(pe);
  }
}

template <typename LP>
hipError_t launch_norms(const LarsArgsOf<LP>& args, const float* grad_coef,
                        const float* skip, float* partials,
                        hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  auto kernel = grad_coef ? lars_norms_k<LP, true> : lars_norms_k<LP, false>;
  kernel<<<grid, block, 0, stream>>>(args, grad_coef, skip, partials);
  return hipGetLastError();
}

template <typename Args>
hipError_t launch_trust(const Args& args, const LarsScalars& s,
                        const float* partials, const float* skip,
                        float* trust, hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  lars_trust_k<Args><<<dim3(args.count), dim3(kTrustThreads), 0, stream>>>(
      args, s, partials, skip, trust);
  return hipGetLastError();
}

template <typename LP>
hipError_t launch_update(const LarsArgsOf<LP>& args, const LarsScalars& s,
                         const float* grad_coef, const float* trust,
                         const float* skip, hipStream_t stream) {
  if (args.count == 0 || args.block_prefix[args.count] == 0) return hipSuccess;
  dim3 grid(args.block_prefix[args.count]), block(kChunkThreads);
  auto kernel =
      s.nesterov ? (grad_coef ? lars_update_k<LP, true, true>
                              : lars_update_k<LP, true, false>)
                 : (grad_coef ? lars_update_k<LP, false, true>
                              : lars_update_k<LP, false, false>);
  kernel<<<grid, block, 0, stream>>>(args, s, grad_coef, trust, skip);
  return hipGetLastError();
}

}  // namespace

hipError_t LarsNormsLaunch(const LarsBatchArgs& args, const float* grad_coef,
                           const float* skip, float* partials,
                           hipStream_t stream) {
  return launch_norms<void>(args, grad_coef, skip, partials, stream);
}

hipError_t LarsTrustLaunch(const LarsBatchArgs& args, const LarsScalars& s,
                           const float* partials, const float* skip,
                           float* trust, hipStream_t stream) {
  return launch_trust(args, s, partials, skip, trust, stream);
}

hipError_t LarsUpdateLaunch(const LarsBatchArgs& args, const LarsScalars& s,
                            const float* grad_coef, const float* trust,
                            const float* skip, hipStream_t stream) {
  return launch_update<void>(args, s, grad_coef, trust, skip, stream);
}

hipError_t LarsNormsMasterLaunch(const LarsMasterBatchArgs& args, int dt,
                                 const float* grad_coef, const float* skip,
                                 float* partials, hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_norms<__half>(args, grad_coef, skip, partials, stream);
    case DT_BF16:
      return launch_norms<__hip_bfloat16>(args, grad_coef, skip, partials,
                                          stream);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t LarsTrustLaunch(const LarsMasterBatchArgs& args,
                           const LarsScalars& s, const float* partials,
                           const float* skip, float* trust,
                           hipStream_t stream) {
  return launch_trust(args, s, partials, skip, trust, stream);
}

hipError_t LarsUpdateMasterLaunch(const LarsMasterBatchArgs& args, int dt,
                                  const LarsScalars& s,
                                  const float* grad_coef, const float* trust,
                                  const float* skip, hipStream_t stream) {
  switch (dt) {
    case DT_F16:
      return launch_update<__half>(args, s, grad_coef, trust, skip, stream);
    case DT_BF16:
      return launch_update<__hip_bfloat16>(args, s, grad_coef, trust, skip,
                                           stream);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace gpu
}  // namespace hvd
