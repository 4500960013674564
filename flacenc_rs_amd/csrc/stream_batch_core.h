// stream_batch_core.h -- the arithmetic of flacenc_hip_decode_streams (flac_decode_streams.cpp) that does not touch a
// frame's bits: which stream a byte position or a frame index belongs to, where a stream's accepted frames end, and the
// checks of the descriptor table.  Shared by the device kernels and the host (tests/host/stream_batch_core_test.cpp
// holds it to brute force under the sanitizers).
//
// A batch is a table of streams in ascending byte order; spans never overlap, gaps between them are legal and a stream
// may be empty.  The frames of all streams are numbered in one sequence, stream after stream in `slot` order (the
// table sorted by channel count, so that the frames of one channel count are one range): base[i] is the number of
// frames in front of slot i, base[n] the total.
#ifndef STREAM_BATCH_CORE_H_
#define STREAM_BATCH_CORE_H_

#include <stdint.h>

#include "flacenc_hip.h"

#if defined(__HIPCC__)
#define SB_HD __host__ __device__ inline
#else
#define SB_HD inline
#endif

namespace streambatch {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MAX_STREAMS = 1u << 24;
constexpr uint64_t MAX_FRAMES = 1ull << 30;

// The stream whose span [offset, offset + n_bytes) holds byte p; NONE for a byte in a gap, in front of the first or
// behind the last stream.  An empty stream holds no byte, wherever it sits.
SB_HD uint32_t stream_of_byte(const flacenc_hip_stream_desc* d, uint32_t n, uint64_t p) {
  uint32_t lo = 0, hi = n;  // the first stream that starts behind p
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (d[mid].offset <= p) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return NONE;
  // spans ascend without overlap: of the streams that start at or before p only the last can reach it
  return p - d[lo - 1].offset < d[lo - 1].n_bytes ? lo - 1 : NONE;
}

// The slot of frame m < base[n]: the last i with base[i] <= m.  Slots without frames share their base with the next
// slot and are never returned.
SB_HD uint32_t slot_of_frame(const uint64_t* base, uint32_t n, uint64_t m) {
  uint32_t lo = 0, hi = n;  // the first slot whose base is above m
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (base[mid] <= m) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// The cut.  pcm[] and bad[] are exclusive prefix sums over the frame sequence: the bytes of PCM a frame decodes to and
// 1 for a frame with a status.  Of the `count` frames from `first` on (one stream's chain) the accepted ones are those
// in front of the first frame that has a status or whose PCM ends beyond `capacity` bytes: both sums only grow, so the
// answer -- how many are accepted, 0..count -- is found by bisection.
SB_HD uint64_t accepted_frames(const uint64_t* pcm, const uint64_t* bad, uint64_t first, uint64_t count,
                               uint64_t capacity) {
  uint64_t lo = 0, hi = count;  // frames [0, lo) are accepted, frame hi (if any) is not
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const bool ok = bad[first + mid + 1] == bad[first] && pcm[first + mid + 1] - pcm[first] <= capacity;
    if (ok) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The descriptor table against the call's buffers: 0, FLACENC_HIP_ERR_BAD_ARGUMENT or FLACENC_HIP_ERR_UNSUPPORTED (the
// first stream that fails decides).  max_bps: the handle's depth limit (flacenc_hip_set_max_bits_per_sample).
inline int check_streams(const flacenc_hip_stream_desc* d, size_t n, uint64_t n_bytes, uint64_t out_bytes,
                         uint32_t max_bps = 24) {
  uint64_t end = 0;  // where the previous span ends
  for (size_t s = 0; s < n; ++s) {
    const flacenc_hip_stream_desc& x = d[s];
    if (x.offset < end || x.n_bytes > n_bytes || x.offset > n_bytes - x.n_bytes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    end = x.offset + x.n_bytes;
    if (x.out_capacity > out_bytes || x.out_offset > out_bytes - x.out_capacity) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.channels < 1 || x.channels > 8 || x.max_block_size < 1 || x.max_block_size > 65536 || x.bytes_per_sample > 4)
      return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.bits_per_sample < 4 || x.bits_per_sample > max_bps) return FLACENC_HIP_ERR_UNSUPPORTED;
    if (x.bytes_per_sample < (x.bits_per_sample + 7) / 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

}  // namespace streambatch

#endif  // STREAM_BATCH_CORE_H_
