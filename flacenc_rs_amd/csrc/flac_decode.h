// flac_decode.h -- launchers of the frame decoder's kernels (flac_decode.cpp) and of the single-stream frame index
// (stream_index.cpp) for api_decode.cpp and api_decode_stream.cpp.
#ifndef FLACENC_FLAC_DECODE_H_
#define FLACENC_FLAC_DECODE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace flacenc_hip {

// scratch of one decode / verify launch of n frames
size_t decode_scratch_bytes(size_t n_frames);

// decode (expected == NULL) or verify (out == NULL) n_frames frames; n_bytes bounds offsets[f] + lengths[f]
// (UINT64_MAX when the caller did not give it); max_bps is the handle's depth limit, here and below
hipError_t launch_decode_frames(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                                const uint32_t* lengths, uint32_t n_frames, uint32_t channels, uint32_t bps,
                                uint32_t max_block_size, uint32_t max_bps, int32_t* out, const int32_t* expected,
                                size_t stride, uint32_t* block_sizes, uint64_t* numbers, uint32_t* status,
                                void* scratch, hipStream_t stream);

// candidate capacity and scratch of one index launch (stream_index.cpp)
size_t index_candidate_capacity(size_t max_frames);
size_t index_scratch_bytes(uint64_t n_bytes, size_t capacity);

hipError_t launch_index_frames(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bps,
                               uint32_t max_bps, size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames,
                               void* scratch, size_t capacity, hipStream_t stream);

// flac_decode.cpp's kernels for the index.  The skim of the single stream [0, n_bytes): frames that start at
// offsets[0 .. min(n, *n_dev)) and may run to n_bytes, their skim records (flacdec::FrameRec) into recs[].  The CRC-16
// of the frames whose record has status 0: FRAME_CRC into the record where it fails.
hipError_t launch_frame_skim(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets, uint32_t n,
                             const uint32_t* n_dev, uint32_t channels, uint32_t bps, uint32_t max_bps, void* recs,
                             hipStream_t stream);
hipError_t launch_frame_crc16(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const uint32_t* n_dev,
                              void* recs, hipStream_t stream);

}  // namespace flacenc_hip

#endif  // FLACENC_FLAC_DECODE_H_
