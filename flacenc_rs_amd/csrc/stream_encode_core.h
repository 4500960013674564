// stream_encode_core.h -- the arithmetic of flacenc_hip_encode_streams (encode_streams.cpp) that runs no analysis: the
// plan (which frame of which stream goes where in which launch) and a fixed-blocking frame rewritten with another frame
// number.  Plain C++, shared by the library and a host build (tests/host/stream_encode_core_test.cpp holds it to brute
// force and to frames the oracle wrote, under the sanitizers).
//
// The plan.  A *class* is (channels, bits_per_sample, bytes_per_sample, sample_rate); classes are numbered in the order
// their first stream appears in the table.  Launch order is class after class; inside a class first every full frame
// (block_size samples) of its streams in table order, then the tails (total_samples % block_size samples) sorted by
// tail length, streams of one length in table order.  So the full frames of a class are one run of rows, and the tails of
// one length are one run: the frame-level calls take one block size per launch.  Stream order is table order, frame after
// frame: the order of frame_lengths.  A frame's launch position p and its stream position q number it in the two orders.
#ifndef STREAM_ENCODE_CORE_H_
#define STREAM_ENCODE_CORE_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flacenc_hip.h"
#include "variable_block_core.h"

namespace streamenc {

constexpr uint32_t MAX_STREAMS = 1u << 24;
constexpr uint64_t MAX_FRAMES = 1ull << 31;  // per stream (the coded frame number) and per call (32-bit positions)

// ---------------------------------------------------------------- a frame packed with number 0, renumbered
// Bytes of a packed frame's header with the coded number `number` in place of the one it has.
FD_HD uint32_t renumbered_header_bytes(const uint8_t* fixed, uint32_t number) {
  const uint32_t hf = vbs::header_bytes(fixed);
  if (hf == 0) return 0;
  uint32_t ones = 0;
  while (ones < 8 && ((fixed[4] >> (7 - ones)) & 1u)) ++ones;
  return hf - (ones == 0 ? 1u : ones) + vbs::coded_number_bytes(number);
}

// The header of the same frame with frame number `number` (< 2^31): the four fixed bytes as they are (fixed blocking
// stays fixed blocking), the new coded number, the block-size / sample-rate bytes as they are, a new CRC-8.  `out` has
// room for 16 bytes; returns the length (4 + 6 + 2 + 2 + 1 at most), 0 for a header vbs::header_bytes rejects.
FD_HD uint32_t write_renumbered_header(const uint8_t* fixed, uint32_t number, uint8_t* out) {
  const uint32_t hf = vbs::header_bytes(fixed);
  if (hf == 0) return 0;
  uint32_t ones = 0;
  while (ones < 8 && ((fixed[4] >> (7 - ones)) & 1u)) ++ones;
  const uint32_t old_num = ones == 0 ? 1u : ones;
  for (uint32_t i = 0; i < 4; ++i) out[i] = fixed[i];
  uint32_t k = 4 + vbs::write_coded_number(out + 4, number);
  for (uint32_t i = 4 + old_num; i + 1 < hf; ++i) out[k++] = fixed[i];
  out[k] = static_cast<uint8_t>(vbs::crc8_bytes(out, k));
  return k + 1;
}

// Length of a frame packed with number 0 once it carries `number`.
FD_HD uint32_t renumbered_length(uint32_t len_at_zero, uint32_t number) {
  return len_at_zero - 1u + vbs::coded_number_bytes(number);
}

// The whole frame, serially (the device moves the body with a workgroup and forms x^(8|B|) across a wave; this is the
// statement both are held to).  `out` has room for len + 5 bytes; returns the new length, 0 for a frame too short to be
// one.
inline uint32_t renumber_frame(const uint8_t* frame, uint32_t len, uint32_t number, uint8_t* out) {
  const uint32_t hf = vbs::header_bytes(frame);
  if (hf == 0 || len < hf + 2u) return 0;
  const uint32_t hv = write_renumbered_header(frame, number, out);
  const uint32_t body = len - 2u - hf;
  for (uint32_t i = 0; i < body; ++i) out[hv + i] = frame[hf + i];
  const uint32_t crc_old = (static_cast<uint32_t>(frame[len - 2]) << 8) | frame[len - 1];
  const uint32_t crc = vbs::crc16_rehead(crc_old, vbs::crc16_bytes(frame, hf), vbs::crc16_bytes(out, hv), body);
  out[hv + body] = static_cast<uint8_t>(crc >> 8);
  out[hv + body + 1] = static_cast<uint8_t>(crc);
  return hv + body + 2u;
}

// ---------------------------------------------------------------- the plan
struct LaunchFrame {     // launch order: what the fill kernel reads
  uint64_t pcm_offset;   // the frame's first byte in `pcm`
  uint32_t valid;        // its samples per channel: block_size, or the tail
  uint32_t stream_pos;   // q, its position in stream order
};
struct StreamFrame {     // stream order: what the place kernel reads
  uint64_t pack_offset;  // the frame's pack slot, in bytes from the start of the pack scratch
  uint32_t launch_pos;   // p
  uint32_t stream;       // its stream's index in the table
  uint32_t index;        // its index within the stream: the frame number it gets
  uint32_t pack_room;    // bytes of that slot: no frame is longer
};
struct Run {             // one frame-level call
  uint32_t first;        // launch position of its first frame
  uint32_t frames;
  uint32_t block;        // the block size it runs at
  uint32_t cls;
};
struct Class {
  uint32_t channels, bits_per_sample, bytes_per_sample, sample_rate;
  uint32_t first;        // launch position of its first frame
  uint32_t full, tails;  // its full frames, then its tails
  uint64_t pack_base;    // its pack slots start here, `pack_stride` bytes each
  uint64_t pack_stride;
};
struct Plan {
  std::vector<LaunchFrame> launch;
  std::vector<StreamFrame> stream;
  std::vector<uint32_t> stream_first;  // [n_streams + 1]: stream s owns stream positions [first[s], first[s + 1])
  std::vector<Class> classes;
  std::vector<Run> runs;               // in launch order: a class's full-frame runs, then its tail runs
  uint32_t full_runs = 0, tail_runs = 0;
  uint64_t pack_bytes = 0;
  uint64_t max_class_rows = 0;         // the largest class, in frames * channels
};

inline uint64_t frames_of(uint64_t total_samples, uint32_t block_size) {
  return total_samples / block_size + (total_samples % block_size ? 1u : 0u);
}

// Sum of ceil(total_samples / block_size); saturates at 2^63 so that no table overflows it.
inline uint64_t count_frames(const flacenc_hip_pcm_stream_desc* d, size_t n, uint32_t block_size) {
  if (!d || block_size == 0) return 0;
  uint64_t sum = 0;
  for (size_t s = 0; s < n; ++s) {
    sum += frames_of(d[s].total_samples, block_size);
    if (sum >= (1ull << 63)) return 1ull << 63;
  }
  return sum;
}

// The table against the call's buffers.  0 or FLACENC_HIP_ERR_BAD_ARGUMENT (overflow-free).  `max_bits` is the handle's
// limit (flacenc_hip_set_max_encode_bits_per_sample), 24 or 32; more than 24 bits come in 4-byte samples.
inline int check_streams(const flacenc_hip_pcm_stream_desc* d, size_t n, uint64_t pcm_bytes, uint64_t out_bytes,
                         uint32_t block_size, uint32_t max_bits = 24) {
  if (block_size < FLACENC_HIP_MIN_BLOCK_SIZE || block_size > FLACENC_HIP_MAX_BLOCK_SIZE) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (size_t s = 0; s < n; ++s) {
    const flacenc_hip_pcm_stream_desc& x = d[s];
    if (x.channels < 1 || x.channels > 8 || x.bytes_per_sample < 1 || x.bytes_per_sample > 4 ||
        x.bits_per_sample < 8 || x.bits_per_sample > max_bits || (x.bits_per_sample > 24 && x.bytes_per_sample != 4))
      return FLACENC_HIP_ERR_BAD_ARGUMENT;
    const uint64_t per = static_cast<uint64_t>(x.channels) * x.bytes_per_sample;
    if (x.total_samples > pcm_bytes / per || x.offset > pcm_bytes - x.total_samples * per) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (x.out_capacity > out_bytes || x.out_offset > out_bytes - x.out_capacity) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (frames_of(x.total_samples, block_size) >= MAX_FRAMES) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

// `chunk_of(class)` >= 1: the most frames one run of that class holds.  `bound(channels, block_size, bits)` is the pack
// slot a frame of a class needs (rounded up to 16 bytes here).  The table has passed check_streams and holds fewer than
// 2^31 frames.
template <typename ChunkOf, typename Bound>
inline Plan build_plan(const flacenc_hip_pcm_stream_desc* d, size_t n, uint32_t block_size, ChunkOf chunk_of, Bound bound) {
  Plan pl;
  std::vector<uint32_t> cls_of(n);
  for (size_t s = 0; s < n; ++s) {
    uint32_t c = 0;
    for (; c < pl.classes.size(); ++c) {
      const Class& k = pl.classes[c];
      if (k.channels == d[s].channels && k.bits_per_sample == d[s].bits_per_sample &&
          k.bytes_per_sample == d[s].bytes_per_sample && k.sample_rate == d[s].sample_rate)
        break;
    }
    if (c == pl.classes.size()) pl.classes.push_back({d[s].channels, d[s].bits_per_sample, d[s].bytes_per_sample, d[s].sample_rate, 0, 0, 0, 0, 0});
    cls_of[s] = c;
    pl.classes[c].full += static_cast<uint32_t>(d[s].total_samples / block_size);
    pl.classes[c].tails += d[s].total_samples % block_size ? 1u : 0u;
  }
  pl.stream_first.resize(n + 1);
  uint32_t q = 0;
  for (size_t s = 0; s < n; ++s) {
    pl.stream_first[s] = q;
    q += static_cast<uint32_t>(frames_of(d[s].total_samples, block_size));
  }
  pl.stream_first[n] = q;
  pl.launch.resize(q);
  pl.stream.resize(q);
  uint32_t p = 0;
  for (Class& k : pl.classes) {
    k.first = p;
    k.pack_base = pl.pack_bytes;
    k.pack_stride = (static_cast<uint64_t>(bound(k.channels, block_size, k.bits_per_sample)) + 15u) & ~15ull;
    pl.pack_bytes += k.pack_stride * (static_cast<uint64_t>(k.full) + k.tails);
    pl.pack_bytes = (pl.pack_bytes + 255u) & ~255ull;
    const uint64_t rows = (static_cast<uint64_t>(k.full) + k.tails) * k.channels;
    if (rows > pl.max_class_rows) pl.max_class_rows = rows;
    p += k.full + k.tails;
  }
  // full frames: per class a running position, streams in table order
  std::vector<uint32_t> at(pl.classes.size());
  for (size_t c = 0; c < pl.classes.size(); ++c) at[c] = pl.classes[c].first;
  auto put = [&](uint32_t pos, size_t s, uint32_t index, uint32_t valid) {
    const Class& k = pl.classes[cls_of[s]];
    const uint64_t per = static_cast<uint64_t>(k.channels) * k.bytes_per_sample;
    const uint32_t sp = pl.stream_first[s] + index;
    pl.launch[pos] = {d[s].offset + static_cast<uint64_t>(index) * block_size * per, valid, sp};
    pl.stream[sp] = {k.pack_base + static_cast<uint64_t>(pos - k.first) * k.pack_stride, pos, static_cast<uint32_t>(s), index,
                      static_cast<uint32_t>(k.pack_stride)};
  };
  for (size_t s = 0; s < n; ++s) {
    const uint32_t full = static_cast<uint32_t>(d[s].total_samples / block_size);
    uint32_t& a = at[cls_of[s]];
    for (uint32_t i = 0; i < full; ++i) put(a++, s, i, block_size);
  }
  // tails: per class sorted by (length, stream)
  std::vector<std::vector<uint64_t>> tails(pl.classes.size());
  for (size_t s = 0; s < n; ++s) {
    const uint32_t t = static_cast<uint32_t>(d[s].total_samples % block_size);
    if (t) tails[cls_of[s]].push_back((static_cast<uint64_t>(t) << 32) | s);
  }
  for (size_t c = 0; c < pl.classes.size(); ++c) {
    const Class& k = pl.classes[c];
    const uint32_t chunk = std::max<uint32_t>(1u, chunk_of(k));
    for (uint32_t f = 0; f < k.full; f += chunk) {
      pl.runs.push_back({k.first + f, std::min(chunk, k.full - f), block_size, static_cast<uint32_t>(c)});
      ++pl.full_runs;
    }
    std::sort(tails[c].begin(), tails[c].end());
    uint32_t pos = k.first + k.full;
    for (size_t i = 0; i < tails[c].size();) {
      const uint32_t t = static_cast<uint32_t>(tails[c][i] >> 32);
      size_t j = i;
      while (j < tails[c].size() && static_cast<uint32_t>(tails[c][j] >> 32) == t) ++j;
      for (size_t f = i; f < j; f += chunk) {
        pl.runs.push_back({pos + static_cast<uint32_t>(f - i), static_cast<uint32_t>(std::min<size_t>(chunk, j - f)), t, static_cast<uint32_t>(c)});
        ++pl.tail_runs;
      }
      for (; i < j; ++i) {
        const size_t s = static_cast<size_t>(tails[c][i] & 0xFFFFFFFFu);
        put(pos++, s, static_cast<uint32_t>(d[s].total_samples / block_size), t);
      }
    }
  }
  return pl;
}

}  // namespace streamenc

#endif  // STREAM_ENCODE_CORE_H_
