// rice_escape.h -- FLACENC_HIP_FLAG_RICE_ESCAPE's post-pass over candidate records (rice_escape.cpp).
#ifndef FLACENC_HIP_RICE_ESCAPE_H_
#define FLACENC_HIP_RICE_ESCAPE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "flacenc_hip.h"

namespace flacenc_hip {

struct RiceEscapeArgs {
  flacenc_hip_subframe_params* params;  // [n_rows] candidate records; status != 0 records are left as they are
  const int32_t* residual;              // row k at residual + k * residual_stride; never written
  size_t residual_stride;
  uint32_t block_size;                  // 64..32767
  uint32_t n_rows;
  uint32_t max_rice_parameter;          // ..=30
  uint32_t finest_only;                 // FLACENC_HIP_FLAG_FINEST_RICE_ORDER
};

hipError_t launch_rice_escape(const RiceEscapeArgs& a, hipStream_t stream);

}  // namespace flacenc_hip
#endif
