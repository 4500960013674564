// stream_recover_core.h -- the arithmetic of flacenc_hip_recover_streams (flac_recover_streams.cpp) that does not touch
// a frame's bits: a frame's coded position, the segmented prefix maximum behind the placement rule, the placement test,
// the cut, the gap in front of a written frame and how a byte range splits into single bytes and 16-byte vectors.
// Shared by the device kernels and the host (tests/host/stream_recover_core_test.cpp holds it to brute force under the
// sanitizers).  The rule itself is stated at flacenc_hip_recover_streams in include/flacenc_hip.h.
#ifndef STREAM_RECOVER_CORE_H_
#define STREAM_RECOVER_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SR_HD __host__ __device__ inline
#else
#define SR_HD inline
#endif

namespace streamrecover {

constexpr uint32_t PIECE = 4096;  // bytes of a gap one workgroup of the zero pass clears

// Rule 3.  P of a frame with the coded `number` (at most 36 bits): the number itself under variable blocking, the
// number times the stream's max_block_size (at most 65536) under fixed blocking.  Fits 64 bits.
SR_HD uint64_t coded_position(uint64_t number, uint32_t variable, uint32_t max_block_size) {
  return variable ? number : number * max_block_size;
}

// What a frame adds to the prefix maximum: its end E = P + block_size, never below the origin (the empty maximum).
SR_HD uint64_t scan_value(uint64_t P, uint32_t block_size, uint64_t origin) {
  const uint64_t E = P + block_size;
  return E > origin ? E : origin;
}

// The operator of the segmented inclusive max-scan: an element is (head, v), head set on a stream's first chain frame.
// combine(a, b), a in front of b, is associative.
struct SegMax {
  uint32_t head;
  uint64_t v;
};
SR_HD SegMax combine(const SegMax& a, const SegMax& b) {
  return {a.head | b.head, b.head ? b.v : (a.v > b.v ? a.v : b.v)};
}

// Rule 4.  prev_max: the maximum of scan_value over all earlier chain frames of the stream, the origin if there is none.
SR_HD bool is_placed(uint64_t P, uint32_t block_size, uint32_t max_block_size, uint64_t origin, uint64_t prev_max) {
  return block_size <= max_block_size && P >= origin && P >= prev_max;
}

// Rule 5.  emax[first .. first + count) is the inclusive prefix maximum of scan_value over one stream's chain frames,
// which only grows.  A placed frame's own end is its emax (it starts at or behind every earlier end), so the placed
// frames that fit a slot of `capacity` bytes, `width` bytes per inter-channel sample, are exactly those in front of the
// first chain frame whose emax lies beyond the slot: that frame's index, 0..count, found by bisection.
SR_HD uint64_t cut_frames(const uint64_t* emax, uint64_t first, uint64_t count, uint64_t origin, uint32_t width,
                          uint64_t capacity) {
  const uint64_t room = capacity / width;  // (E - origin) * W <= capacity  <=>  E - origin <= capacity / W
  uint64_t lo = 0, hi = count;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (emax[first + mid] - origin <= room) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Rule 8.  The silence in front of a written frame at P whose predecessor among the written frames ends at prev_end
// (the origin for the first one): P - prev_end samples from prev_end on; none when 0.
SR_HD uint64_t gap_before(uint64_t P, uint64_t prev_end) { return P - prev_end; }

// the workgroups the zero pass spends on a gap of `bytes` bytes
SR_HD uint64_t pieces_of(uint64_t bytes) { return (bytes + PIECE - 1) / PIECE; }

// The byte range [lo, hi) of addresses as the zero pass writes it: `head` single bytes up to the first 16-byte
// boundary, `vectors` 16-byte stores, `tail` single bytes behind the last boundary.  A range that holds no boundary is
// all head.
struct ZeroSplit {
  uint64_t head, vectors, tail;
};
SR_HD ZeroSplit zero_split(uint64_t lo, uint64_t hi) {
  const uint64_t up = (lo + 15u) & ~static_cast<uint64_t>(15), down = hi & ~static_cast<uint64_t>(15);
  if (up > hi) return {hi - lo, 0, 0};
  return {up - lo, (down - up) / 16, hi - down};  // up <= hi, so up <= down
}

}  // namespace streamrecover

#endif  // STREAM_RECOVER_CORE_H_
