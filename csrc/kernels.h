// Host-visible interface to the CDNA4 kernels (kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ln_philox.h"

namespace hvd {
namespace gpu {

// Matches hvd::DataType codes (common.h) — kept as plain ints so this header
// stays torch-free for the .hip TU.
enum KDType {
  DT_U8 = 0,
  DT_I8 = 1,
  DT_I32 = 2,
  DT_I64 = 3,
  DT_F16 = 4,
  DT_F32 = 5,
  DT_F64 = 6,
  DT_BOOL = 7,
  DT_BF16 = 8,
  DT_U16 = 9,
  DT_I16 = 10,
};

// Descriptor capacity per launch: sized so the by-value kernarg stays well
// under the 4 KB limit (48 * 28 B + 8 ≈ 1.4 KB).
constexpr int kCopyBatchCapacity = 48;

struct CopyBatchArgs {
  const void* src[kCopyBatchCapacity];
  void* dst[kCopyBatchCapacity];
  unsigned long long numel[kCopyBatchCapacity];
  double scale[kCopyBatchCapacity];
  int count = 0;
};

// Batched strided copy with optional per-entry scale and src->dst dtype
// conversion.  grid = count * blocks_per_copy blocks of 256 threads.
hipError_t BatchedCopyLaunch(const CopyBatchArgs& args, int src_dt, int dst_dt,
                             bool with_scale, int blocks_per_copy,
                             hipStream_t stream);

// ---- One-shot xGMI allreduce (oneshot.hip) --------------------------------
// Every rank reads all n peers' staging slots directly over the
// fully-connected xGMI mesh and reduces locally — one step instead of a
// 2(n-1)-hop ring; the win is latency on small/medium buckets.
constexpr int kOneshotMaxRanks = 8;

struct OneshotDeviceArgs {
  // set-local-rank-indexed device pointers, slot-adjusted by the host
  const void* staging[kOneshotMaxRanks];
  void* flags[kOneshotMaxRanks];  // fine-grained uint64 pages
  int n = 0;
  int li = 0;
};

// Spin (1 tiny block) until every rank's consumed counter reaches min_seq —
// my staging slot for the next op is free to overwrite.
hipError_t OneshotWaitConsumedLaunch(const OneshotDeviceArgs& args,
                                     unsigned long long min_seq,
                                     hipStream_t stream);
// Signal ready, wait all ranks, reduce n staging slots into dst (local
// fusion buffer).  bytes must be 16-aligned (fusion padding guarantees it);
// op: 0=sum 1=min 2=max 3=product; dt in {DT_F32,DT_F64,DT_F16,DT_BF16}.
hipError_t OneshotReduceLaunch(const OneshotDeviceArgs& args,
                               unsigned long long seq, int dt,
                               unsigned long long bytes, void* dst, int op,
                               hipStream_t stream);

// ---- Adasum device pipeline (adasum_kernels.hip) ---------------------------
// Stage 1: per-tensor double-precision dot products / squared norms of (a,b)
// pairs; Stage 2: a = acoef*a + bcoef*b with coefficients derived on-device.
struct AdasumBatchArgs {
  void* a[kCopyBatchCapacity];        // dtype = wire dtype
  const void* b[kCopyBatchCapacity];
  unsigned long long numel[kCopyBatchCapacity];
  int count = 0;
};

// dots layout: [count][3] doubles = {dot(a,b), |a|^2, |b|^2}; must be zeroed
// before the dot pass.
hipError_t AdasumDotsLaunch(const AdasumBatchArgs& args, int dt, double* dots,
                            hipStream_t stream);
hipError_t AdasumScaledAddLaunch(const AdasumBatchArgs& args, int dt,
                                 const double* dots, hipStream_t stream);

// ---- Multi-tensor kernels: clip, fused SGD / AdamW / LAMB / LARS -----------
// All take one by-value descriptor batch of at most kCopyBatchCapacity dense
// tensors, filled by multi_tensor.cc: ROWS rows of device pointers (tensor t
// is ptr[row][t]) and the element counts.  SGD and AdamW give every
// descriptor a fixed number of blocks.  The CHUNKED kernels (clip, LAMB, LARS)
// give every block one kChunkElems-element chunk of one tensor:
// block_prefix[t] is the first block of tensor t and block_prefix[count] the
// grid size, so work is balanced by elements whatever the tensor sizes.
constexpr long long kChunkElems = 8192;

inline long long ChunkBlocks(long long numel) {
  return (numel + kChunkElems - 1) / kChunkElems;
}

struct ChunkFields {
  unsigned int block_prefix[kCopyBatchCapacity + 1] = {0};
  // first workspace slot of this launch: block b reduces into slot
  // partial_base + b (a pair of floats for LAMB and LARS)
  unsigned long long partial_base = 0;
};
struct IndexFields {
  // slot of each tensor in a call-wide per-tensor output (the trust array of
  // LAMB and LARS)
  unsigned int out_index[kCopyBatchCapacity];
};
template <int> struct NoFields {};

template <int ROWS, bool CHUNKED, bool INDEXED = false>
struct MultiTensorArgs
    : std::conditional<CHUNKED, ChunkFields, NoFields<0>>::type,
      std::conditional<INDEXED, IndexFields, NoFields<1>>::type {
  static constexpr int kRows = ROWS;
  static constexpr bool kChunked = CHUNKED;
  static constexpr bool kIndexed = INDEXED;
  void* ptr[ROWS][kCopyBatchCapacity];
  unsigned long long numel[kCopyBatchCapacity];
  int count = 0;
};

// Pointer rows.  Gradients are only ever read.
enum MultiTensorRow {
  kRowParam = 0,
  kRowGrad = 1,
  kRowMomentum = 2,  // SGD (null when momentum == 0), LARS
  kRowExpAvg = 2,    // AdamW, LAMB
  kRowExpAvgSq = 3,
  // master-weight kernels: the fp16/bf16 model parameter, written only
  kRowSgdModel = 3,  // SGD, LARS
  kRowModel = 4,  // AdamW, LAMB
};

using ClipBatchArgs = MultiTensorArgs<1, true>;
using SgdBatchArgs = MultiTensorArgs<3, false>;
using AdamwBatchArgs = MultiTensorArgs<4, false>;
using LambBatchArgs = MultiTensorArgs<4, true, true>;
static_assert(sizeof(ClipBatchArgs) == 984 && sizeof(SgdBatchArgs) == 1544 &&
                  sizeof(AdamwBatchArgs) == 1928 && sizeof(LambBatchArgs) == 2328,
              "kernarg bytes of the four structs these replaced");

// Master-weight launches (fp32 master in kRowParam, 2-byte gradient, 2-byte
// model parameter in one more row): by value like the above, so they too must
// stay well under the 4 KB kernarg limit.
using SgdMasterBatchArgs = MultiTensorArgs<4, false>;
using AdamwMasterBatchArgs = MultiTensorArgs<5, false>;
using LambMasterBatchArgs = MultiTensorArgs<5, true, true>;
static_assert(sizeof(SgdMasterBatchArgs) == 1928 &&
                  sizeof(AdamwMasterBatchArgs) == 2312 &&
                  sizeof(LambMasterBatchArgs) == 2712,
              "kernarg bytes: one 384-byte pointer row more than the fp32 "
              "structs, under 4 KB");
using LarsBatchArgs = MultiTensorArgs<3, true, true>;
using LarsMasterBatchArgs = MultiTensorArgs<4, true, true>;
static_assert(sizeof(LarsBatchArgs) == 1944 &&
                  sizeof(LarsMasterBatchArgs) == 2328,
              "kernarg bytes: LAMB's structs less one pointer row, under 4 KB");

// ---- Fused SGD (sgd_kernels.hip) ------------------------------------------
// grad_coef: null, or a device fp32 scalar every gradient element is
// multiplied by (the global-norm clip coefficient, the reciprocal of a loss
// scale, or their product) before weight decay and momentum; the gradients
// themselves are only read.
// skip (every optimizer launch): null, or a device fp32 flag.  Nonzero, the
// whole grid returns after one uniform load and no row is touched; null or
// zero changes nothing in the arithmetic.
hipError_t FusedSgdLaunch(const SgdBatchArgs& args, float lr, float momentum,
                          float weight_decay, float dampening, bool nesterov,
                          const float* grad_coef, const float* skip,
                          hipStream_t stream);
// Master weights: the same kernel instantiated for dt in {DT_F16, DT_BF16}.
// kRowParam holds the fp32 master, kRowGrad a gradient of type dt (widened
// exactly as it is read), kRowSgdModel the model parameter of type dt, which
// receives the updated master rounded to nearest-even.  One dt per launch.
hipError_t FusedSgdMasterLaunch(const SgdMasterBatchArgs& args, int dt,
                                float lr, float momentum, float weight_decay,
                                float dampening, bool nesterov,
                                const float* grad_coef, const float* skip,
                                hipStream_t stream);

// ---- Fused AdamW (adamw_kernels.hip) --------------------------------------
// step is 1-based (bias correction uses beta^step).  grad_coef as in
// FusedSgdLaunch: applied before the moments.
hipError_t FusedAdamwLaunch(const AdamwBatchArgs& args, float lr, float beta1,
                            float beta2, float eps, float weight_decay,
                            long long step, const float* grad_coef,
                            const float* skip, hipStream_t stream);
// Master weights, as FusedSgdMasterLaunch; the model parameter is kRowModel.
hipError_t FusedAdamwMasterLaunch(const AdamwMasterBatchArgs& args, int dt,
                                  float lr, float beta1, float beta2,
                                  float eps, float weight_decay,
                                  long long step, const float* grad_coef,
                                  const float* skip, hipStream_t stream);

// ---- Global-norm gradient clipping (clip_kernels.hip) ----------------------
// Chunked.  One row; tensors are dense, of one dtype per launch (dt in
// {DT_F32, DT_F16, DT_BF16}).
//
// Block b of the launch writes sum(x^2) of its chunk (fp32) to
// partials[args.partial_base + b].
hipError_t MultiSqNormLaunch(const ClipBatchArgs& args, int dt,
                             float* partials, hipStream_t stream);
// Sums partials[0..n) in a fixed order in fp64 (no atomics: bitwise
// reproducible); out[0] = total_norm = sqrt(sum), out[1] = coef =
// min(max_norm / (total_norm + 1e-6), 1) with NaN kept (torch's
// clip_grad_norm_ formula).  n = 0 gives norm 0 and coef min(1e6 * max_norm,
// 1), i.e. 1 unless max_norm < 1e-6.
hipError_t ClipFinalizeLaunch(const float* partials, long long n_partials,
                              float max_norm, float* out, hipStream_t stream);
// The finalize of a loss-scaled step.  Sums the partials exactly as
// ClipFinalizeLaunch does and writes out[4] = {total_norm, coef, found, S}:
//   S          = *p.scale (1 without one): the scale the gradients carry
//   found      = 1 if the fp64 sum is not finite (an inf or NaN element, or
//                finite gradients whose norm passes ~1.8e19) or *p.found_inf
//                is nonzero, else 0
//   total_norm = (float)sqrt(sum) * (1.0f / S), the unscaled norm
//   coef       = clip * (1.0f / S), clip = min(max_norm / (total_norm +
//                1e-6), 1) by ClipFinalizeLaunch's arithmetic, or 1 without
//                has_max_norm
// and then, with p.growth_tracker, updates *p.scale and the tracker in place
// by the rule of torch._amp_update_scale_: on found scale *= backoff and
// tracker = 0; else tracker += 1, and once it is growth_interval, scale *=
// growth if that is finite, and tracker = 0.
struct ScaledFinalizeParams {
  bool has_max_norm = false;
  float max_norm = 0.0f;
  float* scale = nullptr;            // device, 1 element; written only
                                     // with growth_tracker
  const float* found_inf = nullptr;  // device, 1 element
  int* growth_tracker = nullptr;     // device, 1 element; needs scale
  float growth_factor = 1.0f;
  float backoff_factor = 1.0f;
  int growth_interval = 0;
};
hipError_t ScaledClipFinalizeLaunch(const float* partials,
                                    long long n_partials,
                                    const ScaledFinalizeParams& p, float* out,
                                    hipStream_t stream);
// x *= *coef in place; the whole grid returns without touching memory when
// *coef == 1 (but not when it is NaN).
hipError_t MultiScaleLaunch(const ClipBatchArgs& args, int dt,
                            const float* coef, hipStream_t stream);

// ---- Fused LAMB (lamb_kernels.hip) -----------------------------------------
// Chunked.  Three launches per batch, all fp32 (but see the master-weight
// launches below):
//   1. moments + norms: m, v updated in place, u = mhat / (sqrt(vhat) + eps)
//      + weight_decay * p formed in registers; block b writes sum(p^2) and
//      sum(u^2) of its chunk to partials[2 * (partial_base + b) + {0, 1}]
//   2. trust: one block per tensor sums that tensor's slots in a fixed order
//      in fp64 (no atomics: bitwise reproducible) and writes
//      trust[out_index[t]] = |p| / |u| if adapt and both norms are > 0
//      (false for NaN), else 1
//   3. update: p -= lr * trust[out_index[t]] * u, u recomputed from m, v
// With a set skip flag 1. and 3. touch nothing and 2. writes a ratio of 1 for
// each of its tensors without reading the partials.

// Bias correction folded on the host: mhat = m * inv_bc1, sqrt(vhat) =
// sqrt(v) * inv_bc2_sqrt (both 1 without bias correction).
struct LambScalars {
  float lr, beta1, beta2, eps, weight_decay, inv_bc1, inv_bc2_sqrt;
};

// step is 1-based.  grad_coef as in FusedSgdLaunch: applied before the
// moments.
LambScalars LambFoldScalars(float lr, float beta1, float beta2, float eps,
                            float weight_decay, long long step,
                            bool bias_correction);
hipError_t LambMomentsLaunch(const LambBatchArgs& args, const LambScalars& s,
                             const float* grad_coef, const float* skip,
                             float* partials, hipStream_t stream);
hipError_t LambTrustLaunch(const LambBatchArgs& args, const float* partials,
                           bool adapt, const float* skip, float* trust,
                           hipStream_t stream);
hipError_t LambUpdateLaunch(const LambBatchArgs& args, const LambScalars& s,
                            const float* trust, const float* skip,
                            hipStream_t stream);
// Master weights (dt in {DT_F16, DT_BF16}, one per launch): pass 1 reads the
// fp32 master and a gradient of type dt, so norms and trust ratios are the
// master's; pass 3 writes the master and, rounded to nearest-even, the model
// parameter of type dt in kRowModel.
hipError_t LambMomentsMasterLaunch(const LambMasterBatchArgs& args, int dt,
                                   const LambScalars& s,
                                   const float* grad_coef, const float* skip,
                                   float* partials, hipStream_t stream);
hipError_t LambTrustLaunch(const LambMasterBatchArgs& args,
                           const float* partials, bool adapt,
                           const float* skip, float* trust,
                           hipStream_t stream);
hipError_t LambUpdateMasterLaunch(const LambMasterBatchArgs& args, int dt,
                                  const LambScalars& s, const float* trust,
                                  const float* skip, hipStream_t stream);

// ---- Fused LARS (lars_kernels.hip) -----------------------------------------
// Chunked.  Momentum SGD whose step is scaled per tensor by a trust ratio.
// Three launches per batch:
//   1. norms: g' = g * *grad_coef formed as read; block b writes sum(p^2) and
//      sum(g'^2) of its chunk to partials[2 * (partial_base + b) + {0, 1}].
//      Element e of a chunk always goes to lane (e / 4) % 256, accumulator
//      e % 4, in rising order, whatever the alignment and the gradient dtype,
//      so the sums of a master-weight launch are bitwise those of the fp32
//      launch on the widened gradient
//   2. trust: one block per tensor sums that tensor's slots in a fixed order
//      in fp64 (no atomics: bitwise reproducible), wn = |p|, gn = |g'|, and
//      writes trust[out_index[t]] =
//        trust_coefficient * wn / (gn + weight_decay * wn + eps)
//      if adapt and both norms are > 0 (false for NaN), else 1; with
//      trust_clip a ratio r of the first kind becomes r / lr if that is < 1,
//      else 1 (fp32, so lr == 0 gives 1)
//   3. update: d = trust * (g' + weight_decay * p), m = momentum * m + d,
//      p -= lr * (nesterov ? d + momentum * m : m)
// With a set skip flag 1. and 3. touch nothing and 2. writes a ratio of 1 for
// each of its tensors without reading the partials.
struct LarsScalars {
  float lr, momentum, weight_decay, trust_coefficient, eps;
  bool nesterov, trust_clip, adapt;
};

// grad_coef as in FusedSgdLaunch: 1. and 3. both apply it as they read g.
hipError_t LarsNormsLaunch(const LarsBatchArgs& args, const float* grad_coef,
                           const float* skip, float* partials,
                           hipStream_t stream);
hipError_t LarsTrustLaunch(const LarsBatchArgs& args, const LarsScalars& s,
                           const float* partials, const float* skip,
                           float* trust, hipStream_t stream);
hipError_t LarsUpdateLaunch(const LarsBatchArgs& args, const LarsScalars& s,
                            const float* grad_coef, const float* trust,
                            const float* skip, hipStream_t stream);
// Master weights (dt in {DT_F16, DT_BF16}, one per launch): kRowParam holds
// the fp32 master, whose norm 1. takes, kRowGrad a gradient of type dt; 3.
// writes the master and, rounded to nearest-even, the model parameter of type
// dt in kRowSgdModel.
hipError_t LarsNormsMasterLaunch(const LarsMasterBatchArgs& args, int dt,
                                 const float* grad_coef, const float* skip,
                                 float* partials, hipStream_t stream);
hipError_t LarsTrustLaunch(const LarsMasterBatchArgs& args,
                           const LarsScalars& s, const float* partials,
                           const float* skip, float* trust,
                           hipStream_t stream);
hipError_t LarsUpdateMasterLaunch(const LarsMasterBatchArgs& args, int dt,
                                  const LarsScalars& s,
                                  const float* grad_coef, const float* trust,
                                  const float* skip, hipStream_t stream);

// ---- Fused BatchNorm(+Add)+ReLU (bn_kernels.hip) --------------------------
// NHWC dense activations [total=N*H*W rows, C channels], C % 8 == 0,
// dt in {DT_F32, DT_F16, DT_BF16}; stats/params fp32.
//
// The reduction kernels flush block partials into kBnBanks rows of [2*C]
// floats (all zero when the reduction starts): one shared accumulator
// serializes at the memory controller under thousands of blocks.
constexpr int kBnBanks = 64;
// widest layer the fused path takes; sizes the persistent bank workspace
constexpr int kBnMaxChannels = 4096;

// Every activation pointer and per-channel fp32 array below is read as 16-B
// vectors; a launcher returns hipErrorInvalidValue for one that is not 16-B
// aligned (running_mean / running_var are exempt: bn_finalize_k reads them
// one channel per thread).
//
// banks: partial buffer of kBnBanks * 2 * C floats (zeroed): row b holds
// [sum(C), sum of squares(C)] of the blocks with blockIdx % kBnBanks == b.
hipError_t BnStatsLaunch(const void* x, long long total, int C, int dt,
                         float* banks, hipStream_t stream);
// Per-channel forward epilogue in ONE multi-block kernel: fold the banks +
// mean/invstd + running stats.  Replaces ~10 tiny ATen launches per BN layer
// (measured 3.5 ms/step of pure launch overhead at batch 64).
// clear_banks: also write zero to every bank word read (all kBnBanks * 2 * C
// of them), which leaves a persistent workspace ready for the next reduction
// without a memset; mean / invstd must then lie outside the banks.
hipError_t BnFinalizeLaunch(float* banks, float* mean, float* invstd,
                            float* running_mean, float* running_var,
                            long long count, float momentum, float eps,
                            int C, bool clear_banks, hipStream_t stream);
// Reduce banks into sums[0..2C) (the bwd tail; fwd folds it into finalize).
// clear_banks as above; sums lies outside the banks.
hipError_t BnBankReduceLaunch(float* banks, float* sums, int C,
                              bool clear_banks, hipStream_t stream);
hipError_t BnApplyReluLaunch(const void* x, const void* res, void* y,
                             const float* mean, const float* invstd,
                             const float* gamma, const float* beta,
                             long long total, int C, int dt,
                             hipStream_t stream);
// banks as in BnStatsLaunch, rows of [sum(g)(C), sum(g * xhat)(C)] with
// g = dy * (y > 0); a non-null g_out receives g.
// beta != nullptr (layers without a residual; needs gamma, no g_out): y is
// not read, and y > 0 is recomputed bit-exactly from x, mean, invstd, gamma
// and beta as BnApplyReluLaunch stored it.  Otherwise gamma is not read.
hipError_t BnBwdStatsLaunch(const void* x, const void* y, const void* dy,
                            void* g_out, const float* mean,
                            const float* invstd, const float* gamma,
                            const float* beta, long long total, int C, int dt,
                            float* banks, hipStream_t stream);
// beta != nullptr: as above, the pass reads x and dy only.  Otherwise
// y == nullptr: dy is the g that BnBwdStatsLaunch materialized, and the pass
// reads x and g only.
hipError_t BnBwdApplyLaunch(const void* x, const void* y, const void* dy,
                            void* dx, const float* mean, const float* invstd,
                            const float* gamma, const float* beta,
                            const float* sum_g, const float* sum_gx,
                            long long total, int C, int dt, float inv_count,
                            hipStream_t stream);

// ---- SyncBatchNorm (syncbn_kernels.hip) ------------------------------------
// Activations are a dense (outer, C, inner) block: planar (N, C, L) tensors
// pass outer = N, inner = L; channels-last ones pass outer = N*L, inner = 1.
// dt in {DT_F32, DT_F16, DT_BF16}; every statistic and parameter is fp32.
// w / b / running_* may be null.  Needs outer * inner < 2^31 (planar) and
// an element count below 2^24 so the fp32 count word is exact.
//
// True when the reductions of this shape go through a kBnBanks * 2 * C
// float workspace (`banks` below; otherwise it may be null).
bool SyncBnBanked(long long C, long long inner);
// out[2C+1] = [sum(C), sqsum(C), outer*inner]; zeroes what it accumulates
// into, so out (and banks) may come in uninitialised.
hipError_t SyncBnStatsLaunch(const void* x, long long outer, long long C,
                             long long inner, int dt, float* banks, float* out,
                             hipStream_t stream);
// stats = the allreduced [sum, sqsum, count]; the count is read on device.
// var clamps at >= 0; running stats use the unbiased n / max(n-1, 1).
hipError_t SyncBnFinalizeLaunch(const float* stats, float* mean, float* invstd,
                                float* running_mean, float* running_var,
                                float momentum, float eps, int C,
                                hipStream_t stream);
// y = (x - mean) * invstd * w + b
hipError_t SyncBnApplyLaunch(const void* x, void* y, const float* mean,
                             const float* invstd, const float* w,
                             const float* b, long long outer, long long C,
                             long long inner, int dt, hipStream_t stream);
// out[2C] = [sum(dy)(C), sum(dy * xhat)(C)]
hipError_t SyncBnBwdReduceLaunch(const void* x, const void* dy,
                                 const float* mean, const float* invstd,
                                 long long outer, long long C, long long inner,
                                 int dt, float* banks, float* out,
                                 hipStream_t stream);
// dx = w * invstd * (dy - sums[c]/n - xhat * sums[C+c]/n), n = count[0]
hipError_t SyncBnBwdApplyLaunch(const void* x, const void* dy, void* dx,
                                const float* mean, const float* invstd,
                                const float* w, const float* sums,
                                const float* count, long long outer,
                                long long C, long long inner, int dt,
                                hipStream_t stream);

// ---- Fused dropout + residual add + LayerNorm (ln_kernels.hip) -------------
// Rows of H contiguous elements, [M, H]; dt in {DT_F32, DT_F16, DT_BF16} is
// the type T of x, res, y, z, dy, dz and dx.  gamma / beta are fp32
// (*_f32) or T, and may be null (1 and 0).  Statistics and arithmetic are
// fp32.  H % 8 == 0, 8 <= H <= kLnMaxH and every pointer 16-B aligned, or the
// launchers return hipErrorInvalidValue.  The dropout mask is ln_keep8
// (ln_philox.h) of vector row * (H / 8) + col / 8.  No atomics: results are
// bitwise reproducible.
constexpr int kLnMaxH = 4096;

// z = res + keep * scale * x (res may be null), mean / rstd its row
// statistics (variance from the centred values), y = (z - mean) * rstd *
// gamma + beta.  z: null, or receives z rounded to T.
hipError_t LnForwardLaunch(const void* x, const void* res, const void* gamma,
                           bool gamma_f32, const void* beta, bool beta_f32,
                           void* y, void* z, float* mean, float* rstd,
                           long long M, int H, int dt, float eps,
                           const LnDropout& d, hipStream_t stream);
// Partial rows LnBackwardLaunch writes for this shape.
int LnBackwardBlocks(long long M, int H);
// One pass over dy and z: dz = rstd * (g - mean_H(g) - xhat * mean_H(g *
// xhat)), g = dy * gamma, xhat = (z - mean) * rstd; with d.t16 > 0 also
// dx = dz * keep * scale (dx is not touched otherwise).  partials: null, or
// LnBackwardBlocks rows of [2H] fp32; row b receives [sum dy * xhat (H),
// sum dy (H)] over the rows block b visited.
hipError_t LnBackwardLaunch(const void* dy, const void* z, const float* mean,
                            const float* rstd, const void* gamma,
                            bool gamma_f32, void* dz, void* dx,
                            float* partials, long long M, int H, int dt,
                            const LnDropout& d, hipStream_t stream);
// out[0..2H) = the column sums of partials[rows][2H], added in a fixed order.
hipError_t LnFoldLaunch(const float* partials, int rows, int H, float* out,
                        hipStream_t stream);
// out[rows][H] = 1 where the element is kept, else 0.
hipError_t LnKeepMaskLaunch(unsigned char* out, long long rows, int H,
                            const LnDropout& d, hipStream_t stream);

}  // namespace gpu
}  // namespace hvd
