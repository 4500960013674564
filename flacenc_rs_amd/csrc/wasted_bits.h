// wasted_bits.h -- FLACENC_HIP_FLAG_WASTED_BITS (RFC 9639 section 11.25) around the unflagged frame pipelines: a scan
// that finds each subframe signal's wasted bits k, the shifted rows x >> k of the frames that have some, and the
// decision over those rows' candidates (encode_subframe at width w - k, + k bits; try_stereo_coding as usual).
#ifndef FLACENC_HIP_WASTED_BITS_H_
#define FLACENC_HIP_WASTED_BITS_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "flacenc_hip.h"

namespace flacenc_hip {

// Rows of a frame: stereo = the four roles L, R, M = (l + r) >> 1, S = l - r of a 2-channel frame; otherwise the
// `channels` channels of an Independent(n) frame.  Row r of frame f has index f * rows + r in `k`.
struct WastedArgs {
  const int32_t* frames;  // device; channel c of frame f at frames + (f * channels + c) * stride
  size_t stride;
  uint32_t block_size;
  uint32_t n_frames;
  uint32_t channels;  // 2 with stereo
  uint32_t stereo;
  uint32_t bits_per_sample;
  uint8_t* k;         // [n_frames * rows]: the scan's output
  uint32_t* count;    // [1]: frames with any k > 0 (zeroed by the caller before the scan)
  uint32_t* list;     // [n_frames]: those frames, in no particular order
  // fix-up: marked frame i = list[i] for i < m; its row r at shifted + (i * rows + r) * shifted_stride
  uint32_t m;
  int32_t* shifted;
  size_t shifted_stride;
  uint8_t* shifted_bps;  // [m * rows]: w - k
  // the decision over the shifted rows' candidates (index i * rows + r; null when the candidate kind is off)
  uint32_t use_constant, use_fixed, use_lpc, use_leftside, use_rightside, use_midside;
  const flacenc_hip_subframe_params* lpc_params;
  const int32_t* lpc_residual;
  const flacenc_hip_subframe_params* fixed_params;
  const int32_t* fixed_residual;
  const unsigned long long* fixed_keys;
  size_t cand_stride;
  flacenc_hip_stereo_frame_result* results;     // stereo: [n_frames]
  flacenc_hip_channel_result* chan_results;     // otherwise: [n_frames * channels]
  int32_t* residual;  // output row of (frame f, output channel c) at (f * channels + c) * residual_stride
  size_t residual_stride;
};

inline uint32_t wasted_rows(const WastedArgs& a) { return a.stereo ? 4u : a.channels; }

hipError_t launch_wasted_scan(const WastedArgs& a, hipStream_t stream);
hipError_t launch_wasted_shift(const WastedArgs& a, hipStream_t stream);
hipError_t launch_wasted_decide(const WastedArgs& a, hipStream_t stream);

}  // namespace flacenc_hip
#endif
