// stream_planar_core.h -- the layout arithmetic of flacenc_hip_decode_ranges_planar (flac_decode_ranges.cpp) that can be
// stated without the device: a range's planar slot, the address of an element, how an interval of a row splits into a
// scalar head, a body of whole 16-byte vectors and a scalar tail, the interval of a row the zero pass fills, the value
// rule and the check of the range table.  Shared by the device kernels and the host
// (tests/host/stream_planar_core_test.cpp holds it to brute force under the sanitizers).
//
// A slot holds `channels` rows of n_samples 4-byte elements: element (c, i) at out_offset + (c * n_samples + i) * 4.
// out_offset is a multiple of 4 and `out` comes from an allocator, so every element is 4-byte aligned and nothing more:
// a row starts at any of the four residues mod 16.
#ifndef STREAM_PLANAR_CORE_H_
#define STREAM_PLANAR_CORE_H_

#include <stdint.h>
#include <string.h>

#include "flacenc_hip.h"
#include "stream_batch_core.h"

namespace streamplanar {

constexpr uint32_t ELEM = 4;  // bytes of an element in both sample formats

// bytes of the slot of a range of n_samples on a stream of `channels` channels (the caller has checked that it fits)
SB_HD uint64_t slot_bytes(uint32_t channels, uint64_t n_samples) { return static_cast<uint64_t>(channels) * n_samples * ELEM; }

// byte offset of element (c, i) from the start of `out`; row_len is n_samples (the compact staging of the host path
// packs rows of `written` samples instead)
SB_HD uint64_t element_offset(uint64_t slot_offset, uint64_t row_len, uint32_t c, uint64_t i) {
  return slot_offset + (static_cast<uint64_t>(c) * row_len + i) * ELEM;
}

// `count` elements from byte address `addr` (a multiple of 4): `head` elements stored one by one up to the first
// 16-byte boundary, `body` elements (a multiple of 4) stored as whole 16-byte vectors, `tail` elements one by one.
// head + body + tail == count, head <= 3, tail <= 3; nothing outside the interval is touched.
struct Split {
  uint32_t head;
  uint64_t body;
  uint32_t tail;
};
SB_HD Split split(uint64_t addr, uint64_t count) {
  Split s;
  const uint32_t to_boundary = static_cast<uint32_t>((16u - (addr & 15u)) & 15u) / ELEM;  // 0..3
  s.head = count < to_boundary ? static_cast<uint32_t>(count) : to_boundary;
  s.body = (count - s.head) & ~static_cast<uint64_t>(3);
  s.tail = static_cast<uint32_t>(count - s.head - s.body);
  return s;
}

// elements between the last 16-byte boundary at or in front of byte address `addr` (a multiple of 4) and addr: 0..3.
// A writer that stages elements where they lie behind that boundary stores whole vectors from the first boundary on:
// split(addr, count).head == min(count, (4 - lead(addr)) & 3).
SB_HD uint32_t lead(uint64_t addr) { return static_cast<uint32_t>(addr & 15u) / ELEM; }

// the elements of every row that the zero pass fills: [written, n_samples)
struct Interval {
  uint64_t first, count;
};
SB_HD Interval zero_interval(uint64_t written, uint64_t n_samples) {
  Interval z;
  z.first = written < n_samples ? written : n_samples;
  z.count = n_samples - z.first;
  return z;
}

// The value rule.  I32: the reconstructed value.  F32: that value converted to float (round to nearest even), times
// 2^-(bits_per_sample - 1) -- a power of two, so the product is exact; returned as its bit pattern.
SB_HD float scale_of(uint32_t bits_per_sample) {  // bits_per_sample in 1..=32
  const uint32_t u = (127u - (bits_per_sample - 1u)) << 23;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(u);
#else
  memcpy(&f, &u, 4);
#endif
  return f;
}
SB_HD uint32_t element(int32_t value, uint32_t sample_format, float scale) {
  if (sample_format == FLACENC_HIP_SAMPLE_I32) return static_cast<uint32_t>(value);
  const float f = static_cast<float>(value) * scale;
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  memcpy(&u, &f, 4);
#endif
  return u;
}

// The range table against a checked stream table and the output buffer: the rules of streamranges::check_ranges with
// the planar slot, plus out_offset a multiple of 4.  0 or FLACENC_HIP_ERR_BAD_ARGUMENT.
inline int check_ranges(const flacenc_hip_range_desc* r, size_t n, const flacenc_hip_stream_desc* d, size_t n_streams,
                        uint64_t out_bytes) {
  for (size_t i = 0; i < n; ++i) {
    const flacenc_hip_range_desc& x = r[i];
    if (x.stream >= n_streams || x.reserved != 0) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.first_sample + x.n_samples < x.first_sample) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.out_offset % ELEM) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    const uint64_t frame_bytes = static_cast<uint64_t>(d[x.stream].channels) * ELEM;  // 4..32
    if (x.n_samples > out_bytes / frame_bytes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.out_offset > out_bytes - x.n_samples * frame_bytes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

}  // namespace streamplanar

#endif  // STREAM_PLANAR_CORE_H_
