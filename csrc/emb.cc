// Host side of the fused embedding + LayerNorm + dropout kernels
// (emb_kernels.hip), declared in gpu.h.  As in ln.cc: every tensor is
// validated before the first launch, input the kernels do not take raises (no
// ATen fallback), all work goes on torch's current stream with no host
// synchronisation, and the only allocations are the outputs, the fp32 dz
// workspace and the partial rows of the backward.  The stable sort of the ids
// behind the token table's gradient is torch's.
#include "gpu.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "hip_check.h"
#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

[[noreturn]] void EmbFail(const std::string& what) {
  throw std::runtime_error("horovod_amd: fused_emb " + what);
}

int EmbDType(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return DT_F32;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    default: EmbFail("supports fp32, fp16 and bf16 outputs only");
  }
}

// a contiguous, 16-B aligned GPU tensor on ids' device, fp32 or `out`
void CheckDense(const at::Tensor& w, const at::Tensor& ids,
                at::ScalarType out, const char* name) {
  const std::string n(name);
  if (!w.defined() || !w.is_cuda() || w.get_device() != ids.get_device())
    EmbFail("needs GPU tensors on one device (" + n + ")");
  if (w.scalar_type() != at::kFloat && w.scalar_type() != out)
    EmbFail("needs a " + n + " that is fp32 or of the output's dtype");
  if (!w.is_contiguous() || ((uintptr_t)w.data_ptr() % 16) != 0)
    EmbFail("needs contiguous, 16-byte aligned data (" + n + ")");
}

// [rows, H] table; -> rows
int64_t CheckTable(const at::Tensor& w, const at::Tensor& ids, int64_t H,
                   at::ScalarType out, const char* name) {
  CheckDense(w, ids, out, name);
  if (w.dim() != 2 || w.size(1) != H || w.size(0) < 1)
    EmbFail(std::string("needs ") + name + " as a [rows, H] table");
  return w.size(0);
}

bool IsF32(const at::Tensor& t) {
  return !t.defined() || t.scalar_type() == at::kFloat;
}

// Validates every input both passes share and fills the kernels' view of
// them.  weight / bias may be undefined.
EmbTables CheckInputs(const at::Tensor& ids, const at::Tensor& types,
                      const at::Tensor& tok, const at::Tensor& pos,
                      const at::Tensor& typ, const at::Tensor& weight,
                      const at::Tensor& bias, at::ScalarType out) {
  if (!ids.defined() || !ids.is_cuda() || ids.scalar_type() != at::kLong ||
      ids.dim() != 2 || !ids.is_contiguous() || ids.numel() == 0)
    EmbFail("needs input_ids as a contiguous int64 GPU tensor [B, S]");
  if (!tok.defined() || tok.dim() != 2) EmbFail("needs a [V, H] token table");
  const int64_t H = tok.size(1);
  if (H < 8 || H > kLnMaxH || H % 8 != 0)
    EmbFail("needs a row length H with H % 8 == 0 and 8 <= H <= " +
            std::to_string(kLnMaxH) + ", got " + std::to_string(H));
  EmbTables t;
  t.V = CheckTable(tok, ids, H, out, "token table");
  const int64_t P = CheckTable(pos, ids, H, out, "position table");
  const int64_t B = ids.size(0), S = ids.size(1);
  if (S > P)
    EmbFail("got " + std::to_string(S) + " positions for a position table of " +
            std::to_string(P) + " rows");
  if (B > INT32_MAX || P * H > INT32_MAX)
    EmbFail("needs B and the position table's elements below 2^31");
  if (types.defined()) {
    if (!types.is_cuda() || types.get_device() != ids.get_device() ||
        types.scalar_type() != at::kLong || types.sizes() != ids.sizes() ||
        !types.is_contiguous())
      EmbFail("needs token_type_ids like input_ids");
    const int64_t nt = CheckTable(typ, ids, H, out, "type table");
    if (nt > kEmbMaxTypes)
      EmbFail("takes a type table of at most " + std::to_string(kEmbMaxTypes) +
              " rows");
    t.types = (const long long*)types.data_ptr<int64_t>();
    t.typ = typ.data_ptr();
    t.typ_f32 = IsF32(typ);
    t.ntypes = (int)nt;
  }
  for (const at::Tensor* w : {&weight, &bias}) {
    if (!w->defined()) continue;
    CheckDense(*w, ids, out, "LayerNorm parameter");
    if (w->numel() != H) EmbFail("needs LayerNorm parameters of H elements");
  }
  t.ids = (const long long*)ids.data_ptr<int64_t>();
  t.tok = tok.data_ptr();
  t.pos = pos.data_ptr();
  t.gamma = weight.defined() ? weight.data_ptr() : nullptr;
  t.beta = bias.defined() ? bias.data_ptr() : nullptr;
  t.tok_f32 = IsF32(tok);
  t.pos_f32 = IsF32(pos);
  t.gamma_f32 = IsF32(weight);
  t.beta_f32 = IsF32(bias);
  t.B = (int)B;
  t.S = (int)S;
  t.H = (int)H;
  t.P = (int)P;
  return t;
}

LnDropout CheckDropout(double p, uint64_t seed, uint64_t offset) {
  if (!(p >= 0.0 && p <= 1.0)) EmbFail("needs 0 <= p <= 1");
  return LnMakeDropout(p, seed, offset);
}

}  // namespace

std::vector<at::Tensor> FusedEmbForward(at::Tensor ids, at::Tensor types,
                                        at::Tensor tok, at::Tensor pos,
                                        at::Tensor typ, at::Tensor weight,
                                        at::Tensor bias, double p, double eps,
                                        uint64_t seed, uint64_t offset,
                                        at::ScalarType out_dtype) {
  const int dt = EmbDType(out_dtype);
  const EmbTables t =
      CheckInputs(ids, types, tok, pos, typ, weight, bias, out_dtype);
  const LnDropout d = CheckDropout(p, seed, offset);
  const int64_t M = ids.numel();

  const int device = (int)ids.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  at::Tensor y =
      at::empty({t.B, t.S, t.H}, tok.options().dtype(out_dtype));
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(ids.device());
  at::Tensor mean = at::empty({M}, fopts);
  at::Tensor rstd = at::empty({M}, fopts);
  HIP_CHECK(EmbForwardLaunch(t, y.data_ptr(), mean.data_ptr<float>(),
                             rstd.data_ptr<float>(), dt, (float)eps, d,
                             stream));
  return {y, mean, rstd};
}

std::vector<at::Tensor> FusedEmbBackward(at::Tensor dy, at::Tensor ids,
                                         at::Tensor types, at::Tensor tok,
                                         at::Tensor pos, at::Tensor typ,
                                         at::Tensor weight, at::Tensor mean,
                                         at::Tensor rstd, double p,
                                         uint64_t seed, uint64_t offset) {
  if (!dy.defined()) EmbFail("needs dy");
  const int dt = EmbDType(dy.scalar_type());
  const EmbTables t = CheckInputs(ids, types, tok, pos, typ, weight,
                                  at::Tensor(), dy.scalar_type());
  const LnDropout d = CheckDropout(p, seed, offset);
  const int64_t M = ids.numel(), H = t.H;
  if (!dy.is_cuda() || dy.get_device() != ids.get_device() ||
      !dy.is_contiguous() || dy.numel() != M * H || dy.dim() < 1 ||
      dy.size(-1) != H || ((uintptr_t)dy.data_ptr() % 16) != 0)
    EmbFail("needs dy as a contiguous, 16-byte aligned GPU tensor [B, S, H]");
  for (const at::Tensor* s : {&mean, &rstd})
    if (!s->defined() || !s->is_cuda() ||
        s->get_device() != ids.get_device() ||
        s->scalar_type() != at::kFloat || s->numel() != M ||
        !s->is_contiguous())
      EmbFail("needs mean and rstd as contiguous fp32 GPU tensors with one "
              "element per row");

  const int device = (int)ids.get_device();
  c10::hip::HIPGuard guard(device);
  hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
  auto fopts = at::TensorOptions().dtype(at::kFloat).device(ids.device());
  const int chunks = EmbBatchChunks(t.B, t.S, t.H, true);
  const int blocks = EmbPositionBlocks(t.S, t.H) * chunks;
  const int nacc = types.defined() ? 4 : 2;
  at::Tensor dz = at::empty({M, H}, fopts);
  at::Tensor dtok = at::empty({t.V, H}, fopts);
  at::Tensor dpos = at::empty({t.P, H}, fopts);
  at::Tensor sums = at::empty({nacc * H}, fopts);
  // a single chunk, or a single block, writes the result itself
  at::Tensor dpos_part =
      chunks == 1 ? dpos : at::empty({chunks, (int64_t)t.S * H}, fopts);
  at::Tensor wpart = blocks == 1 ? sums : at::empty({blocks, nacc * H}, fopts);
  HIP_CHECK(EmbBackwardLaunch(
      t, dy.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
      dz.data_ptr<float>(), dpos_part.data_ptr<float>(),
      wpart.data_ptr<float>(), chunks, dt, d, stream));
  if (chunks > 1)
    HIP_CHECK(ColumnFoldLaunch(dpos_part.data_ptr<float>(), chunks,
                               (int)(t.S * H), dpos.data_ptr<float>(),
                               stream));
  if (blocks > 1)
    HIP_CHECK(ColumnFoldLaunch(wpart.data_ptr<float>(), blocks,
                               (int)(nacc * H), sums.data_ptr<float>(),
                               stream));
  auto sorted = at::sort(ids.view({-1}), /*stable=*/true, /*dim=*/0,
                         /*descending=*/false);
  HIP_CHECK(EmbScatterLaunch(
      (const long long*)std::get<0>(sorted).data_ptr<int64_t>(),
      (const long long*)std::get<1>(sorted).data_ptr<int64_t>(),
      dz.data_ptr<float>(), dtok.data_ptr<float>(), dpos.data_ptr<float>(), M,
      t.H, t.V, t.S, t.P, stream));
  at::Tensor dtyp;
  if (types.defined())
    dtyp = sums.narrow(0, 2 * H, t.ntypes * H).view({t.ntypes, H});
  return {dtok, dpos, dtyp, sums.narrow(0, 0, H), sums.narrow(0, H, H)};
}

}  // namespace gpu
}  // namespace hvd
