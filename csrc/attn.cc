// Host side of the fused self-attention kernels (attn_kernels.hip), declared
// in gpu.h.  As in ln.cc and gelu.cc: every tensor is validated before the
// first launch, input the kernels do not take raises (no ATen fallback), all
// work goes on torch's current stream with no host synchronisation, and the
// only allocations are the outputs and the [B, heads, S] fp32 row of D_i =
// do_i . o_i that the two backward kernels share.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void AttnFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: fused_attention " + what);
}

bool Aligned16(const at::Tensor& t) {
  return ((uintptr_t)t.data_ptr() % 16) == 0;
}

struct AttnShape {
  int64_t B, S, E, H;
};

// a contiguous, 16-B aligned fp16 / bf16 GPU tensor [B, S, width]
void CheckActivation(const at::Tensor& x, const char* name) {
  const std::string n(name);
  if (!x.defined()) AttnFail("needs " + n);
  if (!x.is_cuda()) AttnFail("needs GPU tensors (" + n + " is not one)");
  if (x.scalar_type() != at::kHalf && x.scalar_type() != at::kBFloat16)
    AttnFail("supports fp16 and bf16 only (" + n + ")");
  if (x.dim() != 3 || !x.is_contiguous())
    AttnFail("needs a contiguous " + n + " of three dimensions");
  if (x.numel() == 0) AttnFail("needs a non-empty " + n);
  if (!Aligned16(x)) AttnFail("needs 16-byte aligned data (" + n + ")");
}

AttnShape CheckQkv(const at::Tensor& qkv, int64_t heads) {
  CheckActivation(qkv, "qkv");
  AttnShape s{qkv.size(0), qkv.size(1), qkv.size(2) / 3, heads};
  if (heads < 1 || heads > 65535 || qkv.size(2) != 3 * kAttnHeadDim * heads)
    AttnFail("needs qkv of [B, S, 3 * 64 * heads] (head dimension 64), got a "
             "last dimension of " + std::to_string(qkv.size(2)) + " for " +
             std::to_string(heads) + " heads");
  if (s.S > kAttnMaxS)
    AttnFail("needs S <= " + std::to_string(kAttnMaxS) + ", got " +
             std::to_string(s.S));
  if (s.B > 65535) AttnFail("needs B <= 65535");
  return s;
}

// [B, S, E] of qkv's dtype and device
void CheckLikeOut(const at::Tensor& t, const at::Tensor& qkv,
                  const AttnShape& s, const char* name) {
  CheckActivation(t, name);
  if (t.get_device() != qkv.get_device() ||
      t.scalar_type() != qkv.scalar_type() || t.size(0) != s.B ||
      t.size(1) != s.S || t.size(2) != s.E)
    AttnFail(std::string("needs ") + name +
             " of [B, S, E] in qkv's dtype, on its device");
}

const unsigned char* CheckMask(const at::Tensor& m, const at::Tensor& qkv,
                               const AttnShape& s) {
  if (!m.defined()) return nullptr;
  if (!m.is_cuda() || m.get_device() != qkv.get_device())
    AttnFail("needs GPU tensors on one device (key_padding_mask)");
  if (m.scalar_type() != at::kBool || m.dim() != 2 || m.size(0) != s.B ||
      m.size(1) != s.S || !m.is_contiguous())
    AttnFail("needs a contiguous bool key_padding_mask of [B, S]");
  return (const unsigned char*)m.data_ptr();
}

LnDropout CheckDropout(double p, uint64_t seed, uint64_t offset) {
  if (!(p >= 0.0 && p <= 1.0)) AttnFail("needs 0 <= p <= 1");
  return LnMakeDropout(p, seed, offset);
}

int DType(const at::Tensor& t) {
  return t.scalar_type() == at::kHalf ? DT_F16 : DT_BF16;
}

}  // namespace

std::vector<at::Tensor> FusedAttentionForward(at::Tensor qkv,
                                              at::Tensor key_padding_mask,
                                              int64_t heads, double p,
                                              uint64_t seed, uint64_t offset) {
  const AttnShape s = CheckQkv(qkv, heads);
  const unsigned char* mask = CheckMask(key_padding_mask, qkv, s);
  const LnDropout d = CheckDropout(p, seed, offset);

  const int device = (int)qkv.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor out = at::empty({s.B, s.S, s.E}, qkv.options());
  at::Tensor lse = at::empty({s.B, s.H, s.S}, qkv.options().dtype(at::kFloat));
  HIP_CHECK(AttnForwardLaunch(qkv.data_ptr(), mask, out.data_ptr(),
                              lse.data_ptr<float>(), s.B, (int)s.S, (int)s.H,
                              DType(qkv), d, stream));
  return {out, lse};
}

at::Tensor FusedAttentionBackward(at::Tensor dout, at::Tensor qkv,
                                  at::Tensor out, at::Tensor lse,
                                  at::Tensor key_padding_mask, int64_t heads,
                                  double p, uint64_t seed, uint64_t offset) {
  const AttnShape s = CheckQkv(qkv, heads);
  CheckLikeOut(dout, qkv, s, "dout");
  CheckLikeOut(out, qkv, s, "out");
  if (!lse.defined() || !lse.is_cuda() ||
      lse.get_device() != qkv.get_device() ||
      lse.scalar_type() != at::kFloat || lse.dim() != 3 ||
      lse.size(0) != s.B || lse.size(1) != s.H || lse.size(2) != s.S ||
      !lse.is_contiguous())
    AttnFail("needs a contiguous fp32 lse of [B, heads, S] on qkv's device");
  const unsigned char* mask = CheckMask(key_padding_mask, qkv, s);
  const LnDropout d = CheckDropout(p, seed, offset);

  const int device = (int)qkv.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor dqkv = at::empty_like(qkv);
  at::Tensor D = at::empty_like(lse);
  HIP_CHECK(AttnBackwardLaunch(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(),
                               lse.data_ptr<float>(), mask, dqkv.data_ptr(),
                               D.data_ptr<float>(), s.B, (int)s.S, (int)s.H,
                               DType(qkv), d, stream));
  return dqkv;
}

}  // namespace gpu
}  // namespace hvd
