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

// ---- Fused BatchNorm+ReLU+MaxPool(3, 2, 1) (bn_pool_kernels.hip) -----------
// The stem: x is NHWC dense [N, H, W, C] under the contract above, with
// N * H * W < 2^31; pooled, gp (its gradient) and codes are NHWC dense
// [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C].  relu(bn(x)) at full resolution
// is never stored.  codes (uint8) holds, per pooled element, kh * 3 + kw of
// its arg-max in the window that starts at (2 * oh - 1, 2 * ow - 1), chosen
// as ATen's max_pool2d chooses it (first maximum in scan order, NaN wins).
// The launchers return hipErrorInvalidValue for a shape outside the contract
// or a pointer that is not 16-B aligned.
//
// pooled = maxpool(relu(bn(x))), bit-equal to BnApplyReluLaunch followed by
// the pool.
hipError_t BnApplyReluPoolLaunch(const void* x, void* pooled,
                                 unsigned char* codes, const float* mean,
                                 const float* invstd, const float* gamma,
                                 const float* beta, long long N, int H, int W,
                                 int C, int dt, hipStream_t stream);
// BnBwdStatsLaunch / BnBwdApplyLaunch with beta (mask recomputed from x),
// where dy is gathered from gp and codes in fp32 instead of read.
hipError_t BnBwdStatsPoolLaunch(const void* x, const void* gp,
                                const unsigned char* codes, const float* mean,
                                const float* invstd, const float* gamma,
                                const float* beta, long long N, int H, int W,
                                int C, int dt, float* banks,
                                hipStream_t stream);
hipError_t BnBwdApplyPoolLaunch(const void* x, const void* gp,
                                const unsigned char* codes, void* dx,
                                const float* mean, const float* invstd,
                                const float* gamma, const float* beta,
                                const float* sum_g, const float* sum_gx,
                                long long N, int H, int W, int C, int dt,
                                float inv_count, hipStream_t stream);

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
// out[0..cols) = the column sums of partials[rows][cols], in the order
// LnFoldLaunch adds them (which is this with cols = 2H).
hipError_t ColumnFoldLaunch(const float* partials, int rows, int cols,
                            float* out, hipStream_t stream);

// ---- Fused bias + GELU + dropout (gelu_kernels.hip) ------------------------
// out = keep * scale * gelu(u + bias) over u of [M, N] contiguous; dt as for
// the LayerNorm kernels is the type T of u, out, dy and du.  bias is [N] fp32
// (bias_f32) or T, or null (0).  tanh picks 0.5 v (1 + tanh(sqrt(2 / pi) (v +
// 0.044715 v^3))) over 0.5 v (1 + erf(v / sqrt 2)).  Arithmetic is fp32 with
// one rounding at the store.  N % 8 == 0, 8 <= N <= kGeluMaxN, M >= 1 and
// every pointer 16-B aligned, or the launchers return hipErrorInvalidValue.
// The dropout mask is ln_keep8 (ln_philox.h) of vector row * (N / 8) +
// col / 8, with d.t16 == 0 an instantiation of its own.  No atomics: results
// are bitwise reproducible.
constexpr int kGeluMaxN = 1 << 30;

// Row chunks (gridDim.y) of a launch for this shape, and the partial rows
// GeluBackwardLaunch writes.
int GeluRowChunks(long long M, int N);
hipError_t GeluForwardLaunch(const void* u, const void* bias, bool bias_f32,
                             void* out, long long M, int N, int dt, bool tanh,
                             const LnDropout& d, hipStream_t stream);
// du = dy * keep * scale * gelu'(u + bias) over `chunks` row chunks.
// partials: null, or [chunks, N] fp32; row c receives the column sums of the
// unrounded du over the rows of chunk c (zeros for an empty chunk).
hipError_t GeluBackwardLaunch(const void* dy, const void* u, const void* bias,
                              bool bias_f32, void* du, float* partials,
                              int chunks, long long M, int N, int dt,
                              bool tanh, const LnDropout& d,
                              hipStream_t stream);

// ---- Fused softmax cross-entropy (xent_kernels.hip) ------------------------
// Rows of V contiguous logits, [M, V]; dt in {DT_F32, DT_F16, DT_BF16} is the
// type T of x and dx, labels are int64, every statistic and all arithmetic is
// fp32.  Only the base pointers of x and dx have to be 16-B aligned: V is
// arbitrary, so a row starts at any multiple of sizeof(T), and the kernels
// peel each row to its own 16-B boundary.  1 <= V <= kXentMaxV, 1 <= M <=
// kXentMaxM and 0 <= eps < 1, or the launchers return hipErrorInvalidValue.
// No atomics: results are bitwise reproducible.
//
// Rows of up to kXentWaveMaxV elements are given one wave each, four rows per
// block; longer rows one 256-thread block each.  At 2048 bf16 elements a lane
// of the wave has exactly the four 16-B loads in flight that the kernels
// unroll to; past that a lone wave would loop where a block's four waves
// still work side by side.
constexpr int kXentWaveMaxV = 2048;
constexpr int kXentMaxV = 1 << 30;
constexpr long long kXentMaxM = 2147483647LL;

// lse[r] = log sum_c exp(x[r, c]); row_loss[r] = lse[r] - (1 - eps) x[r, y_r]
// - (eps / V) sum_c x[r, c], which is F.cross_entropy's label_smoothing; 0
// where y_r == ignore_index, NaN where y_r is neither that nor in [0, V) (such
// a label is never used as an index).
hipError_t XentForwardLaunch(const void* x, const long long* labels,
                             float* lse, float* row_loss, long long M, int V,
                             int dt, float eps, long long ignore_index,
                             hipStream_t stream);
// out[0] = the row losses added in a fixed order, divided with `mean` by
// out[1] = the number of labels that are not ignore_index (0 / 0 = NaN).
hipError_t XentFoldLaunch(const float* row_loss, const long long* labels,
                          long long M, long long ignore_index, bool mean,
                          float* out, hipStream_t stream);
// Column chunks (gridDim.y) the backward cuts the rows of this shape into.
int XentBackwardChunks(long long M, int V, int dt);
// dx[r, c] = g_r (exp(x[r, c] - lse[r]) - (1 - eps) [c == y_r] - eps / V),
// rounded once to T.  reduction 0 (none): g_r = dloss[r]; 1 (mean): dloss[0]
// / count[0]; 2 (sum): dloss[0]; all read on the device.  A row with y_r ==
// ignore_index is written as zeros without reading x; one with a label that
// is neither that nor in [0, V) as NaN.
hipError_t XentBackwardLaunch(const void* x, const long long* labels,
                              const float* lse, const float* dloss,
                              const float* count, void* dx, long long M, int V,
                              int dt, float eps, long long ignore_index,
                              int reduction, hipStream_t stream);

// ---- The same with a bias folded in (xent_bias_kernels.hip) ----------------
// z = x + bias in fp32, bias fp32 [V], takes the place of x in every formula
// above; x, dx, labels, the limits and the reductions are as above, and bias
// has no alignment to keep.  The rows r, r + P, r + 2P, ... start at one
// offset from a 16-B boundary, so they share one cut into head, body vectors
// and tail: they form phase class r mod P.
// P = 16 / gcd(16, (V * sizeof(T)) mod 16): 1, 2, 4 or 8 (at most 4 for fp32).
int XentBiasPhases(int V, int dt);
// Floats between the P shifted copies of the bias the forward reads.
inline long long XentBiasPitch(int V) { return ((long long)V + 3) / 4 * 4; }
// shift: P * XentBiasPitch(V) floats, 16-B aligned, written here by a small
// kernel ahead of the row kernel: copy p holds bias from the first body
// column of class p on, so that a body vector's bias is read in 16-B loads.
// A row with y_r == ignore_index is not read: row_loss[r] = lse[r] = 0.
hipError_t XentBiasForwardLaunch(const void* x, const float* bias,
                                 const long long* labels, float* shift,
                                 float* lse, float* row_loss, long long M,
                                 int V, int dt, float eps,
                                 long long ignore_index, hipStream_t stream);
// Row chunks of each phase class in the backward, which writes P * chunks
// partial rows.
int XentBiasRowChunks(long long M, int V, int dt);
// dx as XentBackwardLaunch with z for x.  partials: [P * chunks, V] fp32, chunks
// = XentBiasRowChunks; row p * chunks + c receives, for every column, the sum
// of the unrounded dx over the rows of chunk c of class p in rising row order
// (zeros for an empty chunk).  Their column sums are dbias.
hipError_t XentBiasBackwardLaunch(const void* x, const float* bias,
                                  const long long* labels, const float* lse,
                                  const float* dloss, const float* count,
                                  void* dx, float* partials, long long M,
                                  int V, int dt, float eps,
                                  long long ignore_index, int reduction,
                                  hipStream_t stream);

// ---- Fused multi-head self-attention (attn_kernels.hip) --------------------
// qkv is the packed in_proj output [B, S, 3E], E = 64 H: q | k | v, head h in
// columns 64h .. 64h + 63 of each; dt in {DT_F16, DT_BF16} is the type T of
// qkv, out, dout and dqkv.  mask: null, or [B, S] bytes, nonzero = padding
// key.  s_ij = 0.125 q_i . k_j, p = softmax over the allowed keys, a = keep *
// scale * p, o = a v.  The dropout mask is ln_keep8 (ln_philox.h) over the
// matrix [B * H * S, S8], S8 = S rounded up to a multiple of 8: element (b,
// h, i, j) is bit j % 8 of vector ((b * H + h) * S + i) * (S8 / 8) + j / 8.
// Statistics and accumulators are fp32; P and dS are rounded to T once, as
// operands of the second product.  1 <= S <= kAttnMaxS, B, H in [1, 65535],
// qkv, out, dout and dqkv 16-B aligned, or the launchers return
// hipErrorInvalidValue.  No atomics: results are bitwise reproducible.
constexpr int kAttnMaxS = 512;
constexpr int kAttnHeadDim = 64;

// out [B, S, E]; lse [B, H, S] = log sum_j exp(s_ij) over the allowed keys.
// A query with no allowed key gets out = 0 and lse = -inf.
hipError_t AttnForwardLaunch(const void* qkv, const unsigned char* mask,
                             void* out, float* lse, long long B, int S, int H,
                             int dt, const LnDropout& d, hipStream_t stream);
// dqkv [B, S, 3E], every element written once, by two kernels: the first
// writes dq and D [B, H, S] (D_i = do_i . o_i, a workspace), the second reads
// D and writes dk and dv.  P is recomputed from lse.
hipError_t AttnBackwardLaunch(const void* dout, const void* qkv,
                              const void* out, const float* lse,
                              const unsigned char* mask, void* dqkv, float* D,
                              long long B, int S, int H, int dt,
                              const LnDropout& d, hipStream_t stream);

// ---- Fused embedding + LayerNorm + dropout (emb_kernels.hip) ---------------
// Row r = b * S + s of ids [B, S]: z = tok[ids_r] + pos[s] (+ typ[types_r]),
// y = keep * scale * (gamma * (z - mean) * rstd + beta), statistics over H in
// fp32.  dt is the type T of y and dy; every table and parameter is fp32
// (its *_f32 flag) or T.  H % 8 == 0, 8 <= H <= kLnMaxH, S <= P, at most
// kEmbMaxTypes type rows and every pointer 16-B aligned, or the launchers
// return hipErrorInvalidValue.  The dropout mask is ln_keep8 (ln_philox.h) of
// vector r * (H / 8) + col / 8.  An id outside [0, V) or a type outside
// [0, ntypes) is clamped before it is used as an index; its row of y is NaN
// and adds nothing to any gradient.  No atomics: results are bitwise
// reproducible.
constexpr int kEmbMaxTypes = 2;

struct EmbTables {
  const long long* ids = nullptr;    // [B, S]
  const long long* types = nullptr;  // [B, S], or null: no type row is added
  const void* tok = nullptr;         // [V, H]
  const void* pos = nullptr;         // [P, H]
  const void* typ = nullptr;         // [ntypes, H]; unused without types
  const void* gamma = nullptr;       // [H], or null (1)
  const void* beta = nullptr;        // [H], or null (0); forward only
  bool tok_f32 = true, pos_f32 = true, typ_f32 = true;
  bool gamma_f32 = true, beta_f32 = true;
  int B = 0, S = 0, H = 0, P = 0, ntypes = 0;
  long long V = 0;
};

// Batch chunks (gridDim.y) of the forward or the backward launch for this
// shape, and the blocks along positions (gridDim.x); the backward writes one
// partial row per block.
int EmbBatchChunks(int B, int S, int H, bool backward);
int EmbPositionBlocks(int S, int H);
// y [B * S, H] of T, mean / rstd [B * S] fp32.
hipError_t EmbForwardLaunch(const EmbTables& t, void* y, float* mean,
                            float* rstd, int dt, float eps,
                            const LnDropout& d, hipStream_t stream);
// Pass one of the backward: dz [B * S, H] fp32, the gradient of z (zeros for
// a row with a bad index).  dpos_part [chunks, S, H] fp32: row c receives the
// sums of dz over the batch entries of chunk c.  wpart [blocks, nacc * H]
// fp32, blocks = EmbPositionBlocks * chunks and nacc = 4 with types, else 2:
// [sum dy keep scale xhat, sum dy keep scale, sum dz of type 0, of type 1]
// over the rows the block visited.
hipError_t EmbBackwardLaunch(const EmbTables& t, const void* dy,
                             const float* mean, const float* rstd, float* dz,
                             float* dpos_part, float* wpart, int chunks,
                             int dt, const LnDropout& d, hipStream_t stream);
// Pass two: dtok [V, H] fp32, row v = the sum of the rows perm[j] of dz over
// the segment of sorted_ids [M] that equals v, in rising j (zeros for an
// empty segment), and rows [S, P) of dpos [P, H] = 0.  sorted_ids / perm are
// the stable sort of ids and its permutation.
hipError_t EmbScatterLaunch(const long long* sorted_ids,
                            const long long* perm, const float* dz,
                            float* dtok, float* dpos, long long M, int H,
                            long long V, int S, int P, hipStream_t stream);

// ---- Compaction of the labelled rows (rows_kernels.hip) --------------------
// A row r of labels [M] (int64) is labelled when labels[r] != ignore_index;
// count is their number.  The kernels compact the labelled rows of x [M, H]
// into rows [capacity, H] in rising position and scatter a gradient back.
// Rows are copied as 16-B vectors whatever their dtype: row_bytes = H *
// sizeof(T), a multiple of 16 up to kRowsMaxRowBytes, 1 <= M, capacity <=
// kRowsMaxM and every pointer 16-B aligned, or the launchers return
// hipErrorInvalidValue.  No host read, no memset, no atomics, no block waits
// for another: results are bitwise reproducible.
constexpr int kRowsChunk = 2048;      // labels per block of the index build
constexpr int kRowsGatherRows = 4;    // output rows per wave of the gather
constexpr long long kRowsMaxM = 2147483647LL;
constexpr long long kRowsMaxRowBytes = 1LL << 24;
// Up to this many chunks the index build is one launch in which the block of
// chunk c counts the c chunks before it; past it a launch of per-chunk counts
// goes first.
constexpr int kRowsRecountMaxChunks = 4;

int RowsIndexChunks(long long M);
// True when RowsIndexLaunch for M labels needs `counts`.
bool RowsIndexUsesCounts(long long M);
// idx [capacity]: the position of the r-th labelled row, -1 in [count,
// capacity).  rank [M]: r for a labelled row (also where r >= capacity), else
// -1.  row_labels [capacity]: the labels of those rows, ignore_index in
// [count, capacity).  count [1]: the number of labelled rows, also when it
// exceeds capacity.  counts: null (one launch, blocks recount), or a
// workspace of RowsIndexChunks(M) ints (two launches).
hipError_t RowsIndexLaunch(const long long* labels, long long M,
                           long long ignore_index, long long capacity,
                           int* counts, int* idx, int* rank,
                           long long* row_labels, int* count,
                           hipStream_t stream);
// rows[r] = x[idx[r]] for r < count, zeros for count <= r < capacity.  With
// count > capacity every element of rows is NaN of dt (DT_F32, DT_F16,
// DT_BF16), as is a row whose idx is outside [0, M).
hipError_t RowsGatherLaunch(const void* x, const int* idx, const int* count,
                            void* rows, long long M, long long capacity,
                            long long row_bytes, int dt, hipStream_t stream);
// dx[r] = d_rows[rank[r]] where 0 <= rank[r] < capacity, else zeros; every
// element of dx [M, H] is written once.
hipError_t RowsScatterLaunch(const void* d_rows, const int* rank, void* dx,
                             long long M, long long capacity,
                             long long row_bytes, hipStream_t stream);

}  // namespace gpu
}  // namespace hvd
