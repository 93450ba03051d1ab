// HIP_CHECK for the host translation units (gpu.cc, multi_tensor.cc).
#pragma once

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>

#define HIP_CHECK(cmd)                                                      \
  do {                                                                      \
    hipError_t e_ = (cmd);                                                  \
    if (e_ != hipSuccess)                                                   \
      throw std::runtime_error(std::string("HIP error: ") +                 \
                               hipGetErrorString(e_) + " at " #cmd);        \
  } while (0)
