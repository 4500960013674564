// flac_decode.h -- launchers of the frame decoder's kernels (flac_decode.cpp) for api_decode.cpp.
#ifndef FLACENC_FLAC_DECODE_H_
#define FLACENC_FLAC_DECODE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace flacenc_hip {

// scratch of one decode / verify launch of n frames
size_t decode_scratch_bytes(size_t n_frames);

// decode (expected == NULL) or verify (out == NULL) n_frames frames; n_bytes bounds offsets[f] + lengths[f]
// (UINT64_MAX when the caller did not give it)
hipError_t launch_decode_frames(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                                const uint32_t* lengths, uint32_t n_frames, uint32_t channels, uint32_t bps,
                                uint32_t max_block_size, int32_t* out, const int32_t* expected, size_t stride,
                                uint32_t* block_sizes, uint64_t* numbers, uint32_t* status, void* scratch,
                                hipStream_t stream);

// candidate capacity and scratch of one index launch
size_t index_candidate_capacity(size_t max_frames);
size_t index_scratch_bytes(uint64_t n_bytes, size_t capacity);

hipError_t launch_index_frames(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bps,
                               size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames,
                               void* scratch, size_t capacity, hipStream_t stream);

// Pieces of the index for the batch index of flac_decode_streams.cpp.  The CRC-16 of frames offsets[0 .. min(n, *n_dev))
// whose skim record (flacdec::FrameRec recs[]) has status 0: FRAME_CRC into the record where it fails.  The jump levels
// 1 .. index_jump_levels(capacity) - 1 from level 0 (jump[0 .. capacity)), level k at jump + k * capacity.
hipError_t launch_frame_crc16(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const uint32_t* n_dev,
                              void* recs, hipStream_t stream);
hipError_t launch_jump_levels(uint32_t* jump, const uint32_t* n_dev, size_t capacity, hipStream_t stream);
uint32_t index_jump_levels(size_t capacity);

}  // namespace flacenc_hip

#endif  // FLACENC_FLAC_DECODE_H_
