// stream_ranges_core.h -- the arithmetic of flacenc_hip_decode_ranges (flac_decode_ranges.cpp) that does not touch a
// frame's bits: which chain frames a range of samples touches, what it may write, its stop reason, the window it takes
// out of one frame and the checks of both tables.  Shared by the device kernels and the host
// (tests/host/stream_ranges_core_test.cpp holds it to brute force under the sanitizers).
//
// Positions count inter-channel samples from the first sample of a stream's span.  They are read off the index's scan
// of PCM bytes over the frame sequence (stream_batch_core.h): frame j of a chain whose first frame is `first` starts at
// (pcm[first + j] - pcm[first]) / frame_bytes, frame_bytes = channels * bytes_per_sample -- the scan of block sizes,
// segmented by subtracting the stream's first entry.
#ifndef STREAM_RANGES_CORE_H_
#define STREAM_RANGES_CORE_H_

#include <stdint.h>

#include "flacenc_hip.h"
#include "stream_batch_core.h"

namespace streamranges {

constexpr uint32_t MAX_RANGES = 1u << 24;

SB_HD uint64_t position(const uint64_t* pcm, uint64_t first, uint64_t j, uint64_t frame_bytes) {
  return (pcm[first + j] - pcm[first]) / frame_bytes;
}

// The chain frame that holds sample p, 0 <= p < position(good): the last j < good with position(j) <= p.
SB_HD uint64_t frame_of_sample(const uint64_t* pcm, uint64_t first, uint64_t good, uint64_t frame_bytes, uint64_t p) {
  uint64_t lo = 0, hi = good;  // the first frame that starts behind p
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (position(pcm, first, mid, frame_bytes) <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

struct Located {
  uint64_t written;  // samples the range gets: [first_sample, first_sample + written)
  uint64_t f0;       // the chain frame that holds first_sample (written or not); `good` when first_sample >= S
  uint64_t frames;   // chain frames f0 .. f0 + frames - 1 are decoded; 0 when nothing is written
};

// A range [a, a + n) (a + n does not overflow) on a stream whose first `good` chain frames decode, S samples in all.
SB_HD Located locate(const uint64_t* pcm, uint64_t first, uint64_t good, uint64_t frame_bytes, uint64_t a, uint64_t n) {
  Located r;
  const uint64_t S = position(pcm, first, good, frame_bytes);
  if (a >= S) {
    r.written = 0;
    r.f0 = good;
    r.frames = 0;
    return r;
  }
  const uint64_t end = a + n < S ? a + n : S;
  r.written = end - a;
  r.f0 = frame_of_sample(pcm, first, good, frame_bytes, a);
  r.frames = r.written ? frame_of_sample(pcm, first, good, frame_bytes, end - 1) - r.f0 + 1 : 0;
  return r;
}

// totals[1] of a range: 0 when all n samples were written, else the stream's own stop reason, else RANGE_END
SB_HD uint64_t stop_reason(uint64_t written, uint64_t n, uint64_t stream_why) {
  return written == n ? 0 : stream_why ? stream_why : FLACENC_HIP_DECODE_RANGE_END;
}

// What a range [a, end) takes out of a frame of bs samples at position pos (the frame holds at least one of them): the
// recurrence runs samples 0 .. skip + take - 1 and stores those from `skip` on; sample skip lands `dst` inter-channel
// samples behind the start of the range's slot.
struct Window {
  uint32_t skip, take;
  uint64_t dst;
};
SB_HD Window window(uint64_t pos, uint32_t bs, uint64_t a, uint64_t end) {
  Window w;
  w.skip = a > pos ? static_cast<uint32_t>(a - pos) : 0u;
  const uint64_t stop = end - pos < bs ? end - pos : bs;
  w.take = static_cast<uint32_t>(stop) - w.skip;
  w.dst = pos + w.skip - a;
  return w;
}

// The stream table as flacenc_hip_decode_ranges reads it: the rules of streambatch::check_streams with out_offset and
// out_capacity ignored.
inline int check_spans(const flacenc_hip_stream_desc* d, size_t n, uint64_t n_bytes, uint32_t max_bps = 24) {
  uint64_t end = 0;
  for (size_t s = 0; s < n; ++s) {
    flacenc_hip_stream_desc x = d[s];
    x.out_offset = x.out_capacity = 0;
    if (x.offset < end) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    const int rc = streambatch::check_streams(&x, 1, n_bytes, 0, max_bps);
    if (rc != FLACENC_HIP_OK) return rc;
    end = x.offset + x.n_bytes;
  }
  return FLACENC_HIP_OK;
}

// The range table against a checked stream table and the output buffer: 0 or FLACENC_HIP_ERR_BAD_ARGUMENT.
inline int check_ranges(const flacenc_hip_range_desc* r, size_t n, const flacenc_hip_stream_desc* d, size_t n_streams,
                        uint64_t out_bytes) {
  for (size_t i = 0; i < n; ++i) {
    const flacenc_hip_range_desc& x = r[i];
    if (x.stream >= n_streams || x.reserved != 0) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.first_sample + x.n_samples < x.first_sample) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    const uint64_t frame_bytes = static_cast<uint64_t>(d[x.stream].channels) * d[x.stream].bytes_per_sample;  // 1..32
    if (x.n_samples > out_bytes / frame_bytes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.out_offset > out_bytes - x.n_samples * frame_bytes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

}  // namespace streamranges

#endif  // STREAM_RANGES_CORE_H_
