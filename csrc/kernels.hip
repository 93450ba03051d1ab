// CDNA4 (gfx950) device kernels for the fusion-buffer data path.
//
// MI355X-native replacement for the reference's cuda_kernels.cu /
// hip_kernels.cu: batched gather/scatter pack/unpack of the
// fusion buffer, with per-entry scaling AND on-the-fly dtype conversion
// fused into the same pass (the reference scales in a separate kernel and
// compresses in Python; here fp16/bf16 wire compression costs zero extra
// HBM traffic).
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
//  * wave64; block = 256 threads (4 waves).
//  * memory-bound: vectorized 16-byte loads per lane (dwordx4), grid-stride.
//  * copies are independent: grid = n_copies * blocks_per_copy so the chip
//    (256 CUs / 8 XCDs) fills even when one tensor dominates.
//  * kernel args passed by value (no H2D staging of descriptor arrays).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include "kernels.h"

namespace hvd {
namespace gpu {

namespace {

template <typename T>
struct AccOf {
  using type = float;
};
template <>
struct AccOf<double> {
  using type = double;
};

template <typename A, typename B>
struct AccOf2 {
  using type =
      typename std::conditional<std::is_same<typename AccOf<A>::type, double>::value ||
                                    std::is_same<typename AccOf<B>::type, double>::value,
                                double, float>::type;
};

// dtype <-> device type mapping (codes match hvd::DataType)
template <typename SrcT, typename DstT, typename AccT>
__device__ __forceinline__ DstT convert_scale(SrcT v, AccT scale) {
  return (DstT)((AccT)v * scale);
}

// no-scale path: a same-type copy returns the value untouched (a bit copy for
// every type, 64-bit integers and fp64 included), an integer pair converts
// as integers, and only a float-family pair goes through fp32
template <typename SrcT, typename DstT>
__device__ __forceinline__ DstT convert_only(SrcT v) {
  if constexpr (std::is_same<SrcT, DstT>::value) {
    return v;
  } else if constexpr (std::is_integral<SrcT>::value &&
                       std::is_integral<DstT>::value) {
    return (DstT)v;
  } else {
    return (DstT)(float)v;
  }
}

template <typename SrcT, typename DstT, bool WITH_SCALE>
__global__ __launch_bounds__(256) void batched_copy_k(CopyBatchArgs args,
                                                      int blocks_per_copy) {
  int copy = blockIdx.x / blocks_per_copy;
  if (copy >= args.count) return;
  const SrcT* __restrict__ src = (const SrcT*)args.src[copy];
  DstT* __restrict__ dst = (DstT*)args.dst[copy];
  const long long n = (long long)args.numel[copy];
  using AccT = typename AccOf2<SrcT, DstT>::type;
  const AccT scale = (AccT)args.scale[copy];

  const long long tid =
      (long long)(blockIdx.x % blocks_per_copy) * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)blocks_per_copy * blockDim.x;

  constexpr int VS = 16 / (int)sizeof(SrcT);  // elems per 16B source chunk
  constexpr int DST_BYTES = VS * (int)sizeof(DstT);

  const bool vec_ok = (((uintptr_t)src & 15) == 0) &&
                      (((uintptr_t)dst & (DST_BYTES >= 16 ? 15 : DST_BYTES - 1)) == 0);
  long long vec_done = 0;
  if (vec_ok) {
    const long long nvec = n / VS;
    vec_done = nvec * VS;
    for (long long i = tid; i < nvec; i += nthreads) {
      union {
        uint4 u;
        SrcT e[VS];
      } in;
      in.u = ((const uint4*)src)[i];
      union {
        unsigned int w[(DST_BYTES + 3) / 4];
        uint2 u2[DST_BYTES >= 8 ? DST_BYTES / 8 : 1];
        uint4 u4[DST_BYTES >= 16 ? DST_BYTES / 16 : 1];
        DstT e[VS];
      } out;
#pragma unroll
      for (int v = 0; v < VS; ++v) {
        if (WITH_SCALE)
          out.e[v] = convert_scale<SrcT, DstT, AccT>(in.e[v], scale);
        else
          out.e[v] = convert_only<SrcT, DstT>(in.e[v]);
      }
      if (DST_BYTES == 32) {
        ((uint4*)dst)[i * 2] = out.u4[0];
        ((uint4*)dst)[i * 2 + 1] = out.u4[1];
      } else if (DST_BYTES == 16) {
        ((uint4*)dst)[i] = out.u4[0];
      } else if (DST_BYTES == 8) {
        ((uint2*)dst)[i] = out.u2[0];
      } else if (DST_BYTES == 4) {
        ((unsigned int*)dst)[i] = out.w[0];
      } else {
#pragma unroll
        for (int v = 0; v < VS; ++v) dst[i * VS + v] = out.e[v];
      }
    }
  }
  for (long long i = vec_done + tid; i < n; i += nthreads) {
    if (WITH_SCALE)
      dst[i] = convert_scale<SrcT, DstT, AccT>(src[i], scale);
    else
      dst[i] = convert_only<SrcT, DstT>(src[i]);
  }
}

// host-side dispatch ---------------------------------------------------------

template <typename SrcT, typename DstT>
hipError_t launch_pair(const CopyBatchArgs& args, bool with_scale, int bpc,
                       hipStream_t stream) {
  dim3 grid(args.count * bpc), block(256);
  if (with_scale)
    batched_copy_k<SrcT, DstT, true><<<grid, block, 0, stream>>>(args, bpc);
  else
    batched_copy_k<SrcT, DstT, false><<<grid, block, 0, stream>>>(args, bpc);
  return hipGetLastError();
}

template <typename SrcT>
hipError_t launch_src(const CopyBatchArgs& args, int dst_dt, bool with_scale,
                      int bpc, hipStream_t stream) {
  switch (dst_dt) {
    case DT_F32: return launch_pair<SrcT, float>(args, with_scale, bpc, stream);
    case DT_F16: return launch_pair<SrcT, __half>(args, with_scale, bpc, stream);
    case DT_BF16:
      return launch_pair<SrcT, __hip_bfloat16>(args, with_scale, bpc, stream);
    case DT_F64: return launch_pair<SrcT, double>(args, with_scale, bpc, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t BatchedCopyLaunch(const CopyBatchArgs& args, int src_dt, int dst_dt,
                             bool with_scale, int blocks_per_copy,
                             hipStream_t stream) {
  if (args.count == 0) return hipSuccess;
  // same-type fast paths (includes all integer types; never scaled)
  if (src_dt == dst_dt && !with_scale) {
    switch (src_dt) {
      case DT_U8:
      case DT_I8:
      case DT_BOOL:
        return launch_pair<unsigned char, unsigned char>(args, false,
                                                         blocks_per_copy, stream);
      case DT_U16:
      case DT_I16:
        return launch_pair<unsigned short, unsigned short>(args, false,
                                                           blocks_per_copy, stream);
      case DT_F16:
        return launch_pair<__half, __half>(args, false, blocks_per_copy, stream);
      case DT_BF16:
        return launch_pair<__hip_bfloat16, __hip_bfloat16>(args, false,
                                                           blocks_per_copy, stream);
      case DT_I32:
        return launch_pair<int, int>(args, false, blocks_per_copy, stream);
      case DT_F32:
        return launch_pair<float, float>(args, false, blocks_per_copy, stream);
      case DT_I64:
        return launch_pair<long long, long long>(args, false, blocks_per_copy,
                                                 stream);
      case DT_F64:
        return launch_pair<double, double>(args, false, blocks_per_copy, stream);
    }
    return hipErrorInvalidValue;
  }
  // int16 tensors travel as int32: RCCL has no 16-bit integer type, and an
  // int32 reduction truncated on unpack equals the wrapping int16 one
  if (!with_scale && src_dt == DT_I16 && dst_dt == DT_I32)
    return launch_pair<short, int>(args, false, blocks_per_copy, stream);
  if (!with_scale && src_dt == DT_I32 && dst_dt == DT_I16)
    return launch_pair<int, short>(args, false, blocks_per_copy, stream);
  // float-family conversions (+ optional scale)
  switch (src_dt) {
    case DT_F32:
      return launch_src<float>(args, dst_dt, with_scale, blocks_per_copy, stream);
    case DT_F16:
      return launch_src<__half>(args, dst_dt, with_scale, blocks_per_copy, stream);
    case DT_BF16:
      return launch_src<__hip_bfloat16>(args, dst_dt, with_scale, blocks_per_copy,
                                        stream);
    case DT_F64:
      return launch_src<double>(args, dst_dt, with_scale, blocks_per_copy, stream);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace gpu
}  // namespace hvd
