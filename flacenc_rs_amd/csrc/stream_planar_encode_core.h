// stream_planar_encode_core.h -- what flacenc_hip_encode_streams_planar (encode_streams_planar.cpp, DESIGN.md section
// 4.23) can state without the device: the quantiser of float32 elements, where the rows of a stream lie in `samples`,
// the check of the table against that buffer, and the layout of the packed image the digests are taken over.  Plain
// C++, shared by the kernels and a host build (tests/host/stream_planar_encode_core_test.cpp holds it to brute force
// under the sanitizers).
//
// Stream s is `channels` rows of 4-byte elements: row c starts at byte offset + c * pitch * 4 of `samples`, elements
// [0, total_samples) of it are its samples; pitch is row_pitch, or total_samples where row_pitch is 0.
#ifndef STREAM_PLANAR_ENCODE_CORE_H_
#define STREAM_PLANAR_ENCODE_CORE_H_

#include <stdint.h>
#include <string.h>

#include "flacenc_hip.h"
#include "stream_batch_core.h"

namespace planarenc {

constexpr uint32_t ELEM = 4;  // bytes of an element in both sample formats

// 2^(bits_per_sample - 1) as a float, bits_per_sample in 1..=32
SB_HD float scale_of(uint32_t bits_per_sample) {
  const uint32_t u = (127u + (bits_per_sample - 1u)) << 23;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(u);
#else
  memcpy(&f, &u, 4);
#endif
  return f;
}

// q(x) = clamp(rne(x * 2^(bits - 1)), -2^(bits - 1), 2^(bits - 1) - 1), the product formed in float32; every NaN is 0.
// `scale` is scale_of(bits) and `hi` the same value as an integer, bits in 8..=24: every bound is a float exactly.
// *clipped is raised by one where the rounded product lay outside the range or x was a NaN.
SB_HD int32_t quantise(float x, float scale, int32_t hi, uint32_t* clipped) {
  const float v = x * scale;
  if (v != v) {
    ++*clipped;
    return 0;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_rintf(v);  // v_rndne_f32: ties to even whatever the rounding mode
#else
  // round to nearest even without <fenv.h>: |v| >= 2^23 is an integer already, below that adding and taking away 2^23
  // rounds in the default mode (the host build never changes it)
  float r = v;
  const float a = v < 0 ? -v : v;
  if (a < 8388608.0f) {
    volatile float t = a + 8388608.0f;
    t = t - 8388608.0f;
    r = v < 0 ? -t : t;
  }
#endif
  const float fhi = static_cast<float>(hi);
  if (r >= fhi) {
    ++*clipped;
    return hi - 1;
  }
  if (r < -fhi) {
    ++*clipped;
    return -hi;
  }
  return static_cast<int32_t>(r);
}

SB_HD float as_float(uint32_t u) {
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(u);
#else
  memcpy(&f, &u, 4);
#endif
  return f;
}

// the sample an element stands for: the element itself, or q of it
SB_HD int32_t sample_of(uint32_t element, uint32_t sample_format, float scale, int32_t hi, uint32_t* clipped) {
  if (sample_format == FLACENC_HIP_SAMPLE_I32) return static_cast<int32_t>(element);
  return quantise(as_float(element), scale, hi, clipped);
}

// the pitch of a stream's rows, in elements
SB_HD uint64_t pitch_of(uint64_t row_pitch, uint64_t total_samples) { return row_pitch ? row_pitch : total_samples; }

// One stream's rows against the buffer, overflow-free: offset a multiple of 4 and inside the buffer, a non-zero
// row_pitch at least total_samples, and the last element of the last row inside samples_bytes.
SB_HD bool rows_inside(uint64_t offset, uint64_t total_samples, uint32_t channels, uint64_t row_pitch,
                       uint64_t samples_bytes) {
  if (offset % ELEM || offset > samples_bytes) return false;
  if (row_pitch && row_pitch < total_samples) return false;
  if (total_samples == 0) return true;  // no element of such a stream exists
  const uint64_t room = (samples_bytes - offset) / ELEM;  // elements from the stream's first to the buffer's end
  if (total_samples > room) return false;
  if (channels <= 1) return true;
  // (channels - 1) * pitch + total_samples <= room
  return pitch_of(row_pitch, total_samples) <= (room - total_samples) / (channels - 1u);
}

// The table against `samples`.  channels is taken as given (streamenc::check_streams holds it to 1..=8 afterwards; a
// count of 0 has no row).  0 or FLACENC_HIP_ERR_BAD_ARGUMENT.
inline int check_rows(const flacenc_hip_pcm_stream_desc* d, size_t n, uint32_t sample_format, uint64_t row_pitch,
                      uint64_t samples_bytes) {
  if (sample_format != FLACENC_HIP_SAMPLE_I32 && sample_format != FLACENC_HIP_SAMPLE_F32) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (size_t s = 0; s < n; ++s)
    if (!rows_inside(d[s].offset, d[s].total_samples, d[s].channels, row_pitch, samples_bytes))
      return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return FLACENC_HIP_OK;
}

// The bytes of `samples` that hold an element of any stream: [first, end); first == end where there is none.  The table
// has passed check_rows.
struct Extent {
  uint64_t first, end;
};
inline Extent extent(const flacenc_hip_pcm_stream_desc* d, size_t n, uint64_t row_pitch) {
  Extent e = {UINT64_MAX, 0};
  for (size_t s = 0; s < n; ++s) {
    if (d[s].total_samples == 0 || d[s].channels == 0) continue;
    const uint64_t last = d[s].offset + ((d[s].channels - 1u) * pitch_of(row_pitch, d[s].total_samples) + d[s].total_samples) * ELEM;
    if (d[s].offset < e.first) e.first = d[s].offset;
    if (last > e.end) e.end = last;
  }
  if (e.first > e.end) e.first = e.end = 0;
  return e;
}

// The packed image: stream s's packed interleaved little-endian PCM, bytes_per_sample bytes a sample, at a 16-byte
// aligned base; the writer stores whole dwords of four sample times, so PACK_SLACK bytes behind a stream's last byte are
// the stream's own too (zero, never hashed).
constexpr uint64_t PACK_SLACK = 16;
SB_HD uint64_t packed_bytes(uint64_t total_samples, uint32_t channels, uint32_t bytes_per_sample) {
  return total_samples * channels * bytes_per_sample;
}
SB_HD uint64_t packed_room(uint64_t packed_len) { return (packed_len + PACK_SLACK + 15u) & ~static_cast<uint64_t>(15); }

// Byte `k` of a stream's packed PCM comes from sample time k / (C*B), channel (k / B) % C, byte k % B of the sample.
struct PackedByte {
  uint64_t t;
  uint32_t c, b;
};
SB_HD PackedByte packed_byte(uint64_t k, uint32_t channels, uint32_t bytes_per_sample) {
  const uint64_t idx = k / bytes_per_sample;
  PackedByte p;
  p.b = static_cast<uint32_t>(k - idx * bytes_per_sample);
  p.t = idx / channels;
  p.c = static_cast<uint32_t>(idx - p.t * channels);
  return p;
}

// What the kernels read per stream (device table) and per frame in launch order.
struct Stream {
  uint64_t elem0;        // element index, from the base the kernels get, of row 0's first element
  uint64_t pitch;        // elements
  uint64_t packed_base;  // byte offset of its packed PCM in the packed image (16-byte aligned)
  uint64_t total_samples;
};
struct Frame {
  uint64_t elem0;  // element index of the frame's first sample in row 0
  uint64_t pitch;
  uint32_t valid;  // its samples per channel
  uint32_t stream;
  uint64_t first;  // its first sample's time in the stream
};

}  // namespace planarenc

#endif  // STREAM_PLANAR_ENCODE_CORE_H_
