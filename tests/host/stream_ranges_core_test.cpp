// stream_ranges_core_test.cpp -- csrc/stream_ranges_core.h against brute force, as a stand-alone program for the address
// and undefined-behaviour sanitizers (tests/test_decode_ranges_cpu.py builds and runs it):
//   locate on random block-size lists, several chains in one frame sequence, with zero-length ranges, ranges that end at,
//     run past and begin beyond the end, against a walk over the samples
//   the window rule: skip, take and destination offsets of every frame a range touches against a per-sample loop
//   the stop reason, and the checks of both tables
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "stream_ranges_core.h"

typedef flacenc_hip_stream_desc Desc;
typedef flacenc_hip_range_desc Range;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      if (++failures > 20) std::exit(1);                              \
    }                                                                 \
  } while (0)

static void test_locate_and_window() {
  std::mt19937_64 rng(0x5EEC);
  for (int round = 0; round < 3000; ++round) {
    // a frame sequence: `front` frames of other streams, this stream's `good` frames, `behind` frames of others
    const uint64_t fb = 1 + rng() % 32, front = rng() % 4, good = rng() % 9, behind = rng() % 3;
    std::vector<uint64_t> bs(front + good + behind), pcm(front + good + behind + 1, 0);
    for (size_t m = 0; m < bs.size(); ++m) {
      bs[m] = rng() % 5 == 0 ? 1 : 1 + rng() % 40;
      pcm[m + 1] = pcm[m] + bs[m] * fb * (m < front ? 3 : 1);  // (other streams have other frame sizes)
    }
    std::vector<uint64_t> frame_of;  // per sample of this stream, its frame
    for (uint64_t j = 0; j < good; ++j)
      for (uint64_t t = 0; t < bs[front + j]; ++t) frame_of.push_back(j);
    const uint64_t S = frame_of.size();
    CHECK(streamranges::position(pcm.data(), front, good, fb) == S);
    for (int k = 0; k < 12; ++k) {
      uint64_t a = rng() % (S + 6), n = rng() % 4 == 0 ? 0 : rng() % (S + 8);
      if (k == 0) a = 0;
      if (k == 1) a = S;
      if (k == 2 && S) { a = S - 1; n = 1; }
      if (k == 3 && S) { a = rng() % S; n = S - a; }  // ends exactly at the end
      if (k == 4) n = ~0ull - a;                       // as long as a range can be
      const streamranges::Located l = streamranges::locate(pcm.data(), front, good, fb, a, n);
      const uint64_t end = a + n < S ? a + n : S;
      const uint64_t written = a < S ? end - a : 0;
      CHECK(l.written == written);
      CHECK(l.f0 == (a < S ? frame_of[a] : good));
      CHECK(l.frames == (written ? frame_of[end - 1] - frame_of[a] + 1 : 0));
      if (a < S) CHECK(streamranges::frame_of_sample(pcm.data(), front, good, fb, a) == frame_of[a]);
      // every frame the range touches: where each of its samples goes, by the window and by a walk
      std::vector<uint64_t> slot(written, ~0ull), hits(written, 0);
      for (uint64_t f = l.f0; f < l.f0 + l.frames; ++f) {
        const uint64_t pos = streamranges::position(pcm.data(), front, f, fb);
        const uint32_t b = static_cast<uint32_t>(bs[front + f]);
        const streamranges::Window w = streamranges::window(pos, b, a, a + written);
        CHECK(w.take >= 1 && w.skip + w.take <= b);
        CHECK(w.skip == (a > pos ? a - pos : 0));
        for (uint32_t t = w.skip; t < w.skip + w.take; ++t) {
          const uint64_t at = w.dst + (t - w.skip);
          CHECK(at < written);
          if (at < written) {
            slot[at] = pos + t;
            ++hits[at];
          }
        }
        // the per-sample rule: sample t of the frame is wanted iff a <= pos + t < end
        for (uint32_t t = 0; t < b; ++t) {
          const bool wanted = pos + t >= a && pos + t < a + written;
          CHECK(wanted == (t >= w.skip && t < w.skip + w.take));
        }
      }
      for (uint64_t i = 0; i < written; ++i) CHECK(hits[i] == 1 && slot[i] == a + i);
    }
  }
}

static void test_stop_reason() {
  CHECK(streamranges::stop_reason(5, 5, 0) == 0);
  CHECK(streamranges::stop_reason(5, 5, FLACENC_HIP_DECODE_CHAIN) == 0);
  CHECK(streamranges::stop_reason(0, 0, FLACENC_HIP_DECODE_CHAIN) == 0);
  CHECK(streamranges::stop_reason(4, 5, 0) == FLACENC_HIP_DECODE_RANGE_END);
  CHECK(streamranges::stop_reason(4, 5, FLACENC_HIP_DECODE_CHAIN) == FLACENC_HIP_DECODE_CHAIN);
  CHECK(streamranges::stop_reason(0, 5, FLACENC_HIP_DECODE_UNSUPPORTED) == FLACENC_HIP_DECODE_UNSUPPORTED);
}

static Desc desc(uint64_t off, uint64_t n, uint32_t channels, uint32_t width) {
  Desc d{};
  d.offset = off;
  d.n_bytes = n;
  d.out_offset = ~0ull;  // never looked at
  d.out_capacity = ~0ull;
  d.channels = channels;
  d.bits_per_sample = 16;
  d.max_block_size = 4096;
  d.bytes_per_sample = width;
  return d;
}

static Range range(uint64_t first, uint64_t n, uint64_t out_offset, uint32_t stream, uint32_t reserved = 0) {
  Range r{};
  r.first_sample = first;
  r.n_samples = n;
  r.out_offset = out_offset;
  r.stream = stream;
  r.reserved = reserved;
  return r;
}

static void test_checks() {
  std::vector<Desc> t{desc(0, 10, 2, 2), desc(10, 0, 1, 2), desc(12, 8, 8, 4)};
  CHECK(streamranges::check_spans(t.data(), t.size(), 20) == FLACENC_HIP_OK);
  CHECK(streamranges::check_spans(t.data(), t.size(), 19) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(streamranges::check_spans(nullptr, 0, 0) == FLACENC_HIP_OK);
  {
    std::vector<Desc> u = t;
    u[2].offset = 9;
    CHECK(streamranges::check_spans(u.data(), u.size(), 20) == FLACENC_HIP_ERR_BAD_ARGUMENT);
    u = t;
    u[1].channels = 9;
    CHECK(streamranges::check_spans(u.data(), u.size(), 20) == FLACENC_HIP_ERR_BAD_ARGUMENT);
    u = t;
    u[0].bits_per_sample = 25;
    u[0].bytes_per_sample = 4;
    CHECK(streamranges::check_spans(u.data(), u.size(), 20) == FLACENC_HIP_ERR_UNSUPPORTED);
  }
  auto one = [&](Range r, uint64_t out_bytes) { return streamranges::check_ranges(&r, 1, t.data(), t.size(), out_bytes); };
  CHECK(one(range(0, 10, 0, 0), 40) == FLACENC_HIP_OK);                        // 10 * 2 * 2 bytes
  CHECK(one(range(0, 10, 1, 0), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);          // one byte past
  CHECK(one(range(0, 10, 0, 0), 39) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(5, 0, 40, 1), 40) == FLACENC_HIP_OK);                        // an empty slot at the very end
  CHECK(one(range(5, 0, 41, 1), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 1, 8, 2), 40) == FLACENC_HIP_OK);                         // 32 bytes a sample
  CHECK(one(range(0, 1, 9, 2), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 1, 0, 3), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);           // no such stream
  CHECK(one(range(0, 1, 0, 0, 1), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);        // reserved
  CHECK(one(range(~0ull, 1, 0, 0), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);       // first + n wraps
  CHECK(one(range(~0ull - 1, 1, 0, 0), 40) == FLACENC_HIP_OK);
  CHECK(one(range(0, ~0ull, 0, 0), ~0ull) == FLACENC_HIP_ERR_BAD_ARGUMENT);    // n * frame bytes wraps
  CHECK(one(range(0, 1, ~0ull, 0), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(streamranges::check_ranges(nullptr, 0, t.data(), t.size(), 0) == FLACENC_HIP_OK);
}

int main() {
  static_assert(sizeof(Range) == 32, "flacenc_hip_range_desc is 32 bytes");
  test_locate_and_window();
  test_stop_reason();
  test_checks();
  if (failures) return 1;
  std::printf("stream_ranges_core OK\n");
  return 0;
}
