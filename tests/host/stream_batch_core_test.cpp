// stream_batch_core_test.cpp -- csrc/stream_batch_core.h against brute force, as a stand-alone program for the address
// and undefined-behaviour sanitizers (tests/test_decode_streams_cpu.py builds and runs it):
//   stream of a byte position: gaps, empty streams (also several at one offset), adjacent streams, every first and last byte
//   slot of a frame index with zero-frame slots in front, between and behind
//   the cut rule against a frame-by-frame walk
//   the checks of the descriptor table
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "stream_batch_core.h"

using streambatch::NONE;
typedef flacenc_hip_stream_desc Desc;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      if (++failures > 20) std::exit(1);                              \
    }                                                                 \
  } while (0)

static Desc desc(uint64_t off, uint64_t n, uint64_t out_off = 0, uint64_t cap = 0) {
  Desc d{};
  d.offset = off;
  d.n_bytes = n;
  d.out_offset = out_off;
  d.out_capacity = cap;
  d.channels = 2;
  d.bits_per_sample = 16;
  d.max_block_size = 4096;
  d.bytes_per_sample = 2;
  return d;
}

static uint32_t brute_stream(const std::vector<Desc>& t, uint64_t p) {
  for (size_t s = 0; s < t.size(); ++s)
    if (p >= t[s].offset && p < t[s].offset + t[s].n_bytes) return static_cast<uint32_t>(s);
  return NONE;
}

static void test_stream_of_byte() {
  std::mt19937_64 rng(0x57EA);
  for (int round = 0; round < 400; ++round) {
    std::vector<Desc> t;
    uint64_t at = rng() % 3;
    const int n = static_cast<int>(rng() % 12);
    for (int s = 0; s < n; ++s) {
      const uint64_t gap = rng() % 4 == 0 ? rng() % 9 : 0;   // mostly adjacent
      const uint64_t len = rng() % 3 == 0 ? 0 : 1 + rng() % 40;  // a third are empty
      at += gap;
      t.push_back(desc(at, len));
      at += len;
    }
    const uint64_t n_bytes = at + rng() % 5;
    CHECK(streambatch::check_streams(t.data(), t.size(), n_bytes, 0) == FLACENC_HIP_OK);
    for (uint64_t p = 0; p < n_bytes + 3; ++p)
      CHECK(streambatch::stream_of_byte(t.data(), static_cast<uint32_t>(t.size()), p) == brute_stream(t, p));
  }
  // no stream at all, and positions far behind the last
  CHECK(streambatch::stream_of_byte(nullptr, 0, 0) == NONE);
  std::vector<Desc> one{desc(16, 4)};
  CHECK(streambatch::stream_of_byte(one.data(), 1, 15) == NONE && streambatch::stream_of_byte(one.data(), 1, 16) == 0);
  CHECK(streambatch::stream_of_byte(one.data(), 1, 19) == 0 && streambatch::stream_of_byte(one.data(), 1, 20) == NONE);
  CHECK(streambatch::stream_of_byte(one.data(), 1, ~0ull) == NONE);
}

static void test_slot_of_frame() {
  std::mt19937_64 rng(0xF4A3E);
  for (int round = 0; round < 400; ++round) {
    const uint32_t n = 1 + static_cast<uint32_t>(rng() % 20);
    std::vector<uint64_t> base(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) base[i + 1] = base[i] + (rng() % 2 ? 0 : rng() % 7);
    for (uint64_t m = 0; m < base[n]; ++m) {
      uint32_t want = NONE;
      for (uint32_t i = 0; i < n; ++i)
        if (base[i] <= m && m < base[i + 1]) want = i;
      CHECK(streambatch::slot_of_frame(base.data(), n, m) == want);
    }
  }
}

static void test_cut() {
  std::mt19937_64 rng(0xC07);
  for (int round = 0; round < 2000; ++round) {
    const uint64_t front = rng() % 5, count = rng() % 14, behind = rng() % 4, total = front + count + behind;
    std::vector<uint64_t> pcm(total + 1, 0), bad(total + 1, 0), size(total), flag(total);
    for (uint64_t m = 0; m < total; ++m) {
      size[m] = 1 + rng() % 64;
      flag[m] = rng() % 9 == 0;
      pcm[m + 1] = pcm[m] + size[m];
      bad[m + 1] = bad[m] + flag[m];
    }
    const uint64_t capacity = rng() % 4 == 0 ? ~0ull : rng() % 500;
    uint64_t want = 0, used = 0;
    while (want < count && !flag[front + want] && size[front + want] <= capacity - used) used += size[front + want++];
    CHECK(streambatch::accepted_frames(pcm.data(), bad.data(), front, count, capacity) == want);
  }
}

static void test_check_streams() {
  std::vector<Desc> t{desc(0, 10, 0, 8), desc(10, 0, 8, 0), desc(10, 5, 8, 8), desc(20, 4, 100, 28)};
  CHECK(streambatch::check_streams(t.data(), t.size(), 24, 128) == FLACENC_HIP_OK);
  CHECK(streambatch::check_streams(t.data(), t.size(), 23, 128) == FLACENC_HIP_ERR_BAD_ARGUMENT);   // past n_bytes
  CHECK(streambatch::check_streams(t.data(), t.size(), 24, 127) == FLACENC_HIP_ERR_BAD_ARGUMENT);   // past out_bytes
  auto with = [&](size_t s, void (*change)(Desc&)) {
    std::vector<Desc> u = t;
    change(u[s]);
    return streambatch::check_streams(u.data(), u.size(), 24, 128);
  };
  CHECK(with(2, [](Desc& d) { d.offset = 9; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);      // overlaps stream 0
  CHECK(with(3, [](Desc& d) { d.offset = 14; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);     // overlaps stream 2
  CHECK(with(1, [](Desc& d) { d.offset = 11; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);     // stream 2 no longer ascends
  CHECK(with(0, [](Desc& d) { d.n_bytes = ~0ull; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);  // offset + n_bytes wraps
  CHECK(with(0, [](Desc& d) { d.offset = ~0ull; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(0, [](Desc& d) { d.out_offset = ~0ull; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(0, [](Desc& d) { d.out_capacity = ~0ull; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.channels = 0; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.channels = 9; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.max_block_size = 0; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.max_block_size = 65537; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.bytes_per_sample = 5; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(with(1, [](Desc& d) { d.bytes_per_sample = 1; }) == FLACENC_HIP_ERR_BAD_ARGUMENT);  // 16 bits in one byte
  CHECK(with(1, [](Desc& d) { d.bits_per_sample = 3; d.bytes_per_sample = 4; }) == FLACENC_HIP_ERR_UNSUPPORTED);
  CHECK(with(1, [](Desc& d) { d.bits_per_sample = 25; d.bytes_per_sample = 4; }) == FLACENC_HIP_ERR_UNSUPPORTED);
  CHECK(with(1, [](Desc& d) { d.bits_per_sample = 32; d.bytes_per_sample = 4; }) == FLACENC_HIP_ERR_UNSUPPORTED);
  CHECK(with(1, [](Desc& d) { d.bits_per_sample = 24; d.bytes_per_sample = 3; }) == FLACENC_HIP_OK);
  CHECK(streambatch::check_streams(nullptr, 0, 0, 0) == FLACENC_HIP_OK);
}

int main() {
  static_assert(sizeof(Desc) == 48, "flacenc_hip_stream_desc is 48 bytes");
  test_stream_of_byte();
  test_slot_of_frame();
  test_cut();
  test_check_streams();
  if (failures) return 1;
  std::printf("stream_batch_core OK\n");
  return 0;
}
