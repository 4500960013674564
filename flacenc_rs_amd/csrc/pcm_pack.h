// pcm_pack.h -- launchers of flacenc_hip_pack_le_bytes' kernels (pcm_pack.cpp) for api_decode_stream.cpp.
#ifndef FLACENC_PCM_PACK_H_
#define FLACENC_PCM_PACK_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace flacenc_hip {

// offsets[f] = sum of min(block_sizes[g], stride) over g < f for f = 0 .. n_frames, total[0] = offsets[n_frames]:
// one workgroup, any n_frames
hipError_t launch_pcm_offsets(const uint32_t* block_sizes, uint64_t n_frames, size_t stride, uint64_t* offsets,
                              uint64_t* total, hipStream_t stream);

// the rows' samples to out + offsets[f] * channels * bytes_per_sample, nothing at all when
// offsets[n_frames] * channels * bytes_per_sample > out_capacity
hipError_t launch_pack_le_bytes(const int32_t* frames, size_t stride, const uint32_t* block_sizes,
                                const uint64_t* offsets, uint64_t n_frames, uint32_t channels,
                                uint32_t bytes_per_sample, uint8_t* out, uint64_t out_capacity, hipStream_t stream);

}  // namespace flacenc_hip

#endif  // FLACENC_PCM_PACK_H_
