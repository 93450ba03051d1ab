// Device helper shared by the fused optimizer step kernels
// (sgd_kernels.hip, adamw_kernels.hip, lamb_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace hvd {
namespace gpu {

// g * coef as a value of its own: the empty asm keeps the compiler from
// contracting the product into a later fma (the weight-decay add, the
// moment updates), so a clip coefficient of exactly 1 reproduces the
// unclipped update bit for bit.
__device__ __forceinline__ float scale_grad(float g, float coef) {
  float r = g * coef;
  asm("" : "+v"(r));
  return r;
}

}  // namespace gpu
}  // namespace hvd
