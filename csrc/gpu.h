// GPU data plane: RCCL over xGMI on a dedicated high-priority HIP stream.
//
// Re-design of the reference's GPUContext/GPUOpContext + NCCL op set
// (horovod/common/ops/gpu_operations.{cc,h} N7, nccl_operations.{cc,h} N8)
// for MI355X: one process per GPU, RCCL as the only backend, torch's HIP
// stream pool for allocator-safe stream interop, pack/unpack through the
// CDNA4 batched-copy kernels (kernels.hip), async completion via a finalizer
// thread.
#pragma once

#include <cstdint>
#include <optional>
#include <vector>

#include <ATen/ATen.h>

namespace hvd {
struct GlobalState;
struct Response;
struct TensorTableEntry;

namespace gpu {

// Record an event on torch's current stream for `device` (the producer
// ordering point the comm stream will wait on).  Returns an opaque handle.
uintptr_t RecordReadyEvent(int device);

// Execute a (possibly fused) response on the GPU.  Asynchronous: entries'
// callbacks fire from the finalizer thread once the comm-stream work is done.
void Execute(GlobalState& st, Response& resp,
             std::vector<TensorTableEntry>& entries);

// Drain the finalizer queue (shutdown path).
void WaitAllPending();
void Shutdown();

// Abort every live RCCL communicator (TCP peer loss, async RCCL error, or
// stall shutdown).  Idempotent; unblocks hung collectives so pending
// handles fail with ABORTED (-> HorovodInternalError) instead of hanging.
// Reference: nccl_operations.cc:56-147 commDestroyOrAbort.
void AbortComms(const std::string& why);
// True once AbortComms ran (cleared by Shutdown for elastic re-init).
bool CommsFailed();

// Autotuner hook: adjust the ring-vs-one-shot crossover at runtime
// (applied rank-synchronously from TUNE responses).
void SetOneshotThreshold(int64_t bytes);

// True once a RCCL communicator has been created (used by tests to assert
// the native path ran).
bool RcclUsed();

// Direct Adasum pairwise combine on torch's current stream:
// a[i] = acoef*a[i] + bcoef*b[i] per tensor (kernel unit-test surface; the
// collective path uses the same kernels inside ExecuteAdasum).
void AdasumCombine(std::vector<at::Tensor>& a, std::vector<at::Tensor>& b);

// Fused BatchNorm(+Add)+ReLU (training forward + backward); see
// bn_kernels.hip.  residual may be undefined.  With beta defined and no
// residual gradient wanted, the backward does not read y (it may be
// undefined): the ReLU mask is recomputed from x.
std::vector<at::Tensor> FusedBnReluForward(at::Tensor x, at::Tensor residual,
                                           at::Tensor gamma, at::Tensor beta,
                                           at::Tensor running_mean,
                                           at::Tensor running_var,
                                           double momentum, double eps);
std::vector<at::Tensor> FusedBnReluBackward(at::Tensor x, at::Tensor y,
                                            at::Tensor dy, at::Tensor mean,
                                            at::Tensor invstd, at::Tensor gamma,
                                            bool need_residual_grad,
                                            at::Tensor beta = at::Tensor());
// False when HOROVOD_FUSED_BN_WORKSPACE=0 selected the per-call banks with
// their memset and the y-reading backward for this process.
bool FusedBnLeanPath();
// One big pass of the fused path on its own (per-pass timing probe):
// which = 0 stats, 1 apply, 2 backward stats, 3 backward apply, 4 / 5 the
// backward passes that recompute the ReLU mask from x; a / b / out may be
// undefined where the pass has no such tensor (see gpu.cc).
void FusedBnPass(int which, at::Tensor x, at::Tensor a, at::Tensor b,
                 at::Tensor out, at::Tensor mean, at::Tensor invstd,
                 at::Tensor gamma, at::Tensor beta);

// SyncBatchNorm passes around the two stats allreduces (syncbn_kernels.hip);
// x is fp32/fp16/bf16, contiguous or channels_last (4-D/5-D).  weight, bias
// and the running stats may be undefined.  All on torch's current stream
// with no host synchronisation.
// -> fp32 [2C+1] = [sum, sqsum, local per-channel count]
at::Tensor SyncBnStats(at::Tensor x);
// stats = allreduced [2C+1]; -> {y, mean, invstd}; updates running stats.
std::vector<at::Tensor> SyncBnNormalize(at::Tensor x, at::Tensor stats,
                                        at::Tensor weight, at::Tensor bias,
                                        at::Tensor running_mean,
                                        at::Tensor running_var,
                                        double momentum, double eps);
// -> fp32 [2C] = [sum(dy), sum(dy * xhat)]
at::Tensor SyncBnBackwardReduce(at::Tensor x, at::Tensor dy, at::Tensor mean,
                                at::Tensor invstd);
// sums = allreduced [2C]; count = 1-element fp32 device tensor (global n).
at::Tensor SyncBnBackwardApply(at::Tensor x, at::Tensor dy, at::Tensor mean,
                               at::Tensor invstd, at::Tensor weight,
                               at::Tensor sums, at::Tensor count);

// ---- Fused dropout + residual add + LayerNorm; defined in ln.cc ------------
// y = LayerNorm(residual + dropout(x)) over the last dimension H of a
// contiguous x (ln_kernels.hip): H % 8 == 0, 8 <= H <= 4096, fp32 / fp16 /
// bf16, every tensor 16-B aligned and on one GPU; residual (x's shape and
// dtype), weight and bias (fp32 or x's dtype) may be undefined.  Anything
// else throws before the first launch.  The dropout mask is a function of
// (seed, offset, element index) alone, see ln_philox.h; p is quantised to
// 1/65536.
// -> {y, z, mean, rstd}: z = residual + dropout(x) rounded to x's dtype, only
// with save_z and when it is not x itself (else undefined); mean / rstd fp32,
// one per row.
std::vector<at::Tensor> FusedLnForward(at::Tensor x, at::Tensor residual,
                                       at::Tensor weight, at::Tensor bias,
                                       double p, double eps, uint64_t seed,
                                       uint64_t offset, bool save_z);
// z: what the forward returned, or its x where that was undefined.
// -> {dz, dx, dgamma, dbeta}: dz is the residual's gradient, dx = dz * keep *
// scale (the same tensor as dz when p quantises to 0); dgamma / dbeta fp32
// [H], undefined without need_wgrad.  Bitwise reproducible.
std::vector<at::Tensor> FusedLnBackward(at::Tensor dy, at::Tensor z,
                                        at::Tensor mean, at::Tensor rstd,
                                        at::Tensor weight, double p,
                                        uint64_t seed, uint64_t offset,
                                        bool need_wgrad);
// uint8 [rows, H], 1 where the element is kept: the mask function evaluated
// on the host (CPU device) or in a kernel.  For tests.
at::Tensor FusedLnKeepMask(int64_t rows, int64_t H, double p, uint64_t seed,
                           uint64_t offset, c10::Device device);

// ---- Multi-tensor kernels; defined in multi_tensor.cc ----------------------
// Global-norm clipping (clip_kernels.hip) on torch's current stream with no
// host synchronisation.  grads: dense fp32/fp16/bf16 tensors of one GPU, any
// number of them.  -> fp32 [2] = {total_norm, coef}, coef =
// min(max_norm / (total_norm + 1e-6), 1) as torch.nn.utils.clip_grad_norm_;
// bitwise reproducible for identical inputs.  An empty list gives norm 0,
// hence coef 1 by that formula unless max_norm < 1e-6.
at::Tensor MultiTensorGradNorm(std::vector<at::Tensor>& grads,
                               double max_norm);
// The norm pass of a loss-scaled step (scaled_clip_finalize_k): the same
// multi-tensor pass over gradients that still carry the loss scale S, then
// -> fp32 [4] = {total_norm, coef, found, S}.  S = *scale (1 without one);
// total_norm is the unscaled norm; coef = clip / S with clip the coefficient
// above for the unscaled norm (1 without max_norm), i.e. what a step kernel
// multiplies the scaled gradient by; found = 1 when the sum of squares is not
// finite or *found_inf is nonzero, else 0, in the form the steps take as
// `skip`.  With growth_tracker, *scale and the tracker are then updated in
// place by the rule of torch._amp_update_scale_.  scale, found_inf: undefined
// or 1-element fp32 tensors on the gradients' device; growth_tracker:
// undefined or 1-element int32, and needs a scale.  Everything is checked
// before the first launch.
at::Tensor MultiTensorScaledGradNorm(
    std::vector<at::Tensor>& grads, std::optional<double> max_norm,
    at::Tensor scale = at::Tensor(), at::Tensor found_inf = at::Tensor(),
    at::Tensor growth_tracker = at::Tensor(), double growth_factor = 1.0,
    double backoff_factor = 1.0, int64_t growth_interval = 0);
// tensors[i] *= coef in place; coef is a 1-element fp32 device tensor.
void MultiTensorScale(std::vector<at::Tensor>& tensors, at::Tensor coef);

// The steps below take dense fp32 tensors of one GPU, lists of one
// length, a parameter's tensors of one size and layout; anything else throws
// before the first launch.  An empty tensor is skipped.
//
// Fused SGD step on torch's current stream (one launch per 48 tensors;
// `momenta` is read only when momentum != 0).  grad_coef: undefined, or a
// 1-element fp32 device tensor the kernel multiplies every gradient element
// by as it reads it (the gradients are not written).
//
// model_params (all three steps): null, or the fp16/bf16 model parameters of
// a master-weight step.  `params` are then their fp32 masters, the moments
// stay fp32, grads[i] has the dtype of model_params[i] (fp16 and bf16 may mix
// within a call; each takes launches of its own), every tuple has one size,
// device and layout, and the kernels write the updated master, rounded to
// nearest-even, into the model parameter.
//
// skip (all three steps): undefined, or a 1-element fp32 device tensor.  When
// it is nonzero the kernels return without touching any tensor (and the LAMB
// trust ratios are all 1); the host does not learn of it.  Undefined or zero
// gives the results of a call without it, bit for bit.
void FusedSgdStep(std::vector<at::Tensor>& params,
                  std::vector<at::Tensor>& grads,
                  std::vector<at::Tensor>& momenta, double lr, double momentum,
                  double weight_decay, double dampening, bool nesterov,
                  at::Tensor grad_coef = at::Tensor(),
                  const std::vector<at::Tensor>* model_params = nullptr,
                  at::Tensor skip = at::Tensor());

// Fused AdamW step (decoupled weight decay, torch.optim.AdamW math);
// step is the 1-based step count for bias correction.  grad_coef as in
// FusedSgdStep.
void FusedAdamwStep(std::vector<at::Tensor>& params,
                    std::vector<at::Tensor>& grads,
                    std::vector<at::Tensor>& exp_avgs,
                    std::vector<at::Tensor>& exp_avg_sqs, double lr,
                    double beta1, double beta2, double eps,
                    double weight_decay, int64_t step,
                    at::Tensor grad_coef = at::Tensor(),
                    const std::vector<at::Tensor>* model_params = nullptr,
                    at::Tensor skip = at::Tensor());

// Fused LAMB step (lamb_kernels.hip): AdamW's moments, then per tensor
// p -= lr * trust * u with u = mhat / (sqrt(vhat) + eps) + weight_decay * p
// and trust = |p| / |u| when `adapt` and both norms are > 0, else 1.
// Without bias_correction mhat = m and vhat = v.  Three launches per 48
// tensors on torch's current stream, no host synchronisation.  -> fp32
// [params.size()], the trust ratio applied to each parameter (1 for an empty
// one); bitwise reproducible for identical inputs.  grad_coef as in
// FusedSgdStep.
at::Tensor FusedLambStep(std::vector<at::Tensor>& params,
                         std::vector<at::Tensor>& grads,
                         std::vector<at::Tensor>& exp_avgs,
                         std::vector<at::Tensor>& exp_avg_sqs, double lr,
                         double beta1, double beta2, double eps,
                         double weight_decay, int64_t step,
                         bool bias_correction, bool adapt,
                         at::Tensor grad_coef = at::Tensor(),
                         const std::vector<at::Tensor>* model_params = nullptr,
                         at::Tensor skip = at::Tensor());

// Fused LARS step (lars_kernels.hip), under the rules of the three steps
// above (`momenta` is always read and written).  With g' = g * grad_coef, per
// tensor:
//   trust = trust_coefficient * |p| / (|g'| + weight_decay * |p| + eps) when
//           `adapt` and both norms are > 0, else 1; with trust_clip such a
//           ratio becomes min(trust / lr, 1)
//   d = trust * (g' + weight_decay * p),  m = momentum * m + d,
//   p -= lr * (nesterov ? d + momentum * m : m)
// Three launches per 48 tensors on torch's current stream, no host
// synchronisation.  -> fp32 [params.size()], the trust ratio applied to each
// parameter (1 for an empty one, and for every one when skip is set); bitwise
// reproducible for identical inputs, and with model_params bitwise the
// masters, momenta and ratios of the fp32 step on the widened gradients.
at::Tensor FusedLarsStep(std::vector<at::Tensor>& params,
                         std::vector<at::Tensor>& grads,
                         std::vector<at::Tensor>& momenta, double lr,
                         double momentum, double weight_decay,
                         double trust_coefficient, double eps, bool nesterov,
                         bool trust_clip, bool adapt,
                         at::Tensor grad_coef = at::Tensor(),
                         const std::vector<at::Tensor>* model_params = nullptr,
                         at::Tensor skip = at::Tensor());

}  // namespace gpu
}  // namespace hvd
