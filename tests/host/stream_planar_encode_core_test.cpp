// stream_planar_encode_core_test.cpp -- csrc/stream_planar_encode_core.h against brute force, built with
// -fsanitize=address,undefined (tests/test_encode_streams_planar_cpu.py builds and runs it):
//   * rows_inside / check_rows against the same rule in 128-bit integers, on small buffers exhaustively and at the
//     2^64 boundaries where a 64-bit product or sum would wrap; pitch 0 against the same stream at pitch = total_samples
//   * extent against a walk over every valid element
//   * packed_byte / packed_bytes / packed_room against the three nested loops that write packed PCM
//   * quantise against the rule in double (a float times a power of two is exact there; nearbyint rounds to nearest
//     even) on ties around both clamp edges and 0 with their float neighbours, +-0, denormals, +-1, 1 - ulp, +-FLT_MAX,
//     +-inf, quiet and signalling NaNs, at 8, 16, 20 and 24 bits; and q(v * 2^-(bits-1)) == v for every v of 8 and 16 bits
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_planar_encode_core.h"

using u128 = unsigned __int128;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
      if (++failures > 20) std::exit(1);                            \
    }                                                               \
  } while (0)

static bool brute_inside(uint64_t offset, uint64_t total, uint32_t channels, uint64_t row_pitch, uint64_t bytes) {
  if (offset % 4 || offset > bytes) return false;
  if (row_pitch && row_pitch < total) return false;
  if (total == 0) return true;
  const u128 pitch = row_pitch ? row_pitch : total;
  const u128 last = static_cast<u128>(offset) + (static_cast<u128>(channels - 1) * pitch + total) * 4;
  return channels == 0 ? static_cast<u128>(offset) + static_cast<u128>(total) * 4 <= bytes : last <= bytes;
}

static void test_rows() {
  // exhaustive on small numbers
  for (uint64_t bytes = 0; bytes <= 70; ++bytes)
    for (uint64_t offset = 0; offset <= 72; ++offset)
      for (uint64_t total = 0; total <= 6; ++total)
        for (uint32_t c = 1; c <= 4; ++c)
          for (uint64_t pitch = 0; pitch <= 8; ++pitch)
            CHECK(planarenc::rows_inside(offset, total, c, pitch, bytes) == brute_inside(offset, total, c, pitch, bytes));
  // pitch 0 is the stream's own length
  for (uint64_t total = 1; total <= 9; ++total)
    for (uint32_t c = 1; c <= 8; ++c)
      for (uint64_t bytes = 0; bytes <= 8 * 9 * 4 + 8; bytes += 4)
        CHECK(planarenc::rows_inside(4, total, c, 0, bytes) == planarenc::rows_inside(4, total, c, total, bytes));
  // the 2^64 boundaries: products and sums that wrap in 64 bits
  const uint64_t M = UINT64_MAX;
  const uint64_t big[] = {0, 1, 4, 8, (1ull << 32) - 4, 1ull << 32, (1ull << 61), (1ull << 62) - 1, (1ull << 62), (1ull << 62) + 1,
                          (1ull << 63) - 4, 1ull << 63, M / 4, M / 4 + 1, M / 8, M / 8 + 1, M - 3, M - 7, M & ~3ull, M};
  for (uint64_t bytes : big)
    for (uint64_t offset : big)
      for (uint64_t total : big)
        for (uint64_t pitch : big)
          for (uint32_t c : {1u, 2u, 3u, 8u})
            CHECK(planarenc::rows_inside(offset, total, c, pitch, bytes) == brute_inside(offset, total, c, pitch, bytes));
  // the row's end against samples_bytes, to the byte
  CHECK(planarenc::rows_inside(8, 5, 3, 7, 8 + (2 * 7 + 5) * 4));
  CHECK(!planarenc::rows_inside(8, 5, 3, 7, 8 + (2 * 7 + 5) * 4 - 1));
  CHECK(planarenc::rows_inside(8, 5, 3, 0, 8 + 15 * 4));
  CHECK(!planarenc::rows_inside(8, 5, 3, 0, 8 + 15 * 4 - 1));
  CHECK(!planarenc::rows_inside(6, 5, 1, 0, 1000));   // offset no multiple of 4
  CHECK(!planarenc::rows_inside(8, 5, 1, 4, 1000));   // pitch below the length
  CHECK(planarenc::rows_inside(1000, 0, 8, 0, 1000) && !planarenc::rows_inside(1004, 0, 8, 0, 1000));

  flacenc_hip_pcm_stream_desc d[3];
  std::memset(d, 0, sizeof d);
  d[0].offset = 0, d[0].total_samples = 4, d[0].channels = 2;
  d[1].offset = 64, d[1].total_samples = 0, d[1].channels = 1;
  d[2].offset = 32, d[2].total_samples = 3, d[2].channels = 3;
  CHECK(planarenc::check_rows(d, 3, FLACENC_HIP_SAMPLE_I32, 0, 68) == FLACENC_HIP_OK);
  CHECK(planarenc::check_rows(d, 3, FLACENC_HIP_SAMPLE_F32, 0, 67) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(planarenc::check_rows(d, 3, 2, 0, 68) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(planarenc::check_rows(d, 3, FLACENC_HIP_SAMPLE_F32, 3, 1000) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(planarenc::check_rows(d, 0, FLACENC_HIP_SAMPLE_F32, 3, 0) == FLACENC_HIP_OK);
  // extent: a walk over every valid element
  for (uint64_t pitch : {0ull, 4ull, 9ull}) {
    uint64_t first = UINT64_MAX, end = 0;
    for (int s = 0; s < 3; ++s)
      for (uint32_t c = 0; c < d[s].channels; ++c)
        for (uint64_t i = 0; i < d[s].total_samples; ++i) {
          const uint64_t at = d[s].offset + (c * planarenc::pitch_of(pitch, d[s].total_samples) + i) * 4;
          if (at < first) first = at;
          if (at + 4 > end) end = at + 4;
        }
    const planarenc::Extent e = planarenc::extent(d, 3, pitch);
    CHECK(e.first == first && e.end == end);
  }
  const planarenc::Extent none = planarenc::extent(d + 1, 1, 0);
  CHECK(none.first == none.end);
}

static void test_packed() {
  for (uint32_t C = 1; C <= 8; ++C)
    for (uint32_t B = 1; B <= 4; ++B) {
      uint64_t k = 0;
      for (uint64_t t = 0; t < 7; ++t)
        for (uint32_t c = 0; c < C; ++c)
          for (uint32_t b = 0; b < B; ++b, ++k) {
            const planarenc::PackedByte p = planarenc::packed_byte(k, C, B);
            CHECK(p.t == t && p.c == c && p.b == b);
          }
      CHECK(planarenc::packed_bytes(7, C, B) == k);
      const planarenc::PackedByte far = planarenc::packed_byte((((1ull << 40) + 3) * C + (C - 1)) * B + (B - 1), C, B);
      CHECK(far.t == (1ull << 40) + 3 && far.c == C - 1 && far.b == B - 1);   // past 32 bits
    }
  for (uint64_t n = 0; n < 100; ++n) {
    const uint64_t r = planarenc::packed_room(n);
    CHECK(r % 16 == 0 && r >= n + planarenc::PACK_SLACK && r < n + planarenc::PACK_SLACK + 16);
    CHECK(((n + 3) / 4) * 4 <= r);   // the writer's last whole dword
  }
}

static int32_t brute_q(float x, uint32_t bits, bool* clipped) {
  const double lo = -std::ldexp(1.0, bits - 1), hi = std::ldexp(1.0, bits - 1) - 1;
  *clipped = false;
  if (std::isnan(x)) {
    *clipped = true;
    return 0;
  }
  const double r = std::nearbyint(std::ldexp(static_cast<double>(x), bits - 1));   // exact product, ties to even
  if (r > hi) return *clipped = true, static_cast<int32_t>(hi);
  if (r < lo) return *clipped = true, static_cast<int32_t>(lo);
  return static_cast<int32_t>(r);
}

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static void test_quantise() {
  for (uint32_t bits : {8u, 16u, 20u, 24u}) {
    const float scale = planarenc::scale_of(bits);
    const int32_t top = 1 << (bits - 1);
    CHECK(scale == std::ldexp(1.0f, bits - 1));
    std::vector<float> xs;
    for (int64_t centre : {static_cast<int64_t>(-top), static_cast<int64_t>(0), static_cast<int64_t>(top - 1)})
      for (int64_t k = centre - 3; k <= centre + 3; ++k)
        for (double h : {-0.5, 0.0, 0.5}) {
          const float t = static_cast<float>((static_cast<double>(k) + h) / std::ldexp(1.0, bits - 1));
          xs.push_back(t);
          xs.push_back(std::nextafterf(t, INFINITY));
          xs.push_back(std::nextafterf(t, -INFINITY));
        }
    const float one_less = std::nextafterf(1.0f, 0.0f);
    for (float v : {0.0f, -0.0f, 1.0f, -1.0f, one_less, -one_less, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, FLT_MIN, -FLT_MIN})
      xs.push_back(v);
    for (uint32_t u : {0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x00400000u, 0x7FC00000u, 0xFFC00000u,
                       0x7F800001u, 0xFF800001u, 0x7FBFFFFFu, 0xFFFFFFFFu})
      xs.push_back(from_bits(u));
    for (float x : xs) {
      bool want_clip;
      const int32_t want = brute_q(x, bits, &want_clip);
      uint32_t clipped = 5;
      const int32_t got = planarenc::quantise(x, scale, top, &clipped);
      CHECK(got == want && clipped == 5u + want_clip);
      uint32_t bitsx;
      std::memcpy(&bitsx, &x, 4);
      uint32_t c2 = 0;
      CHECK(planarenc::sample_of(bitsx, FLACENC_HIP_SAMPLE_F32, scale, top, &c2) == want && c2 == want_clip);
      CHECK(planarenc::sample_of(bitsx, FLACENC_HIP_SAMPLE_I32, scale, top, &c2) == static_cast<int32_t>(bitsx) && c2 == want_clip);
    }
    // the inverse of the decoder's rule
    const int64_t step = bits <= 16 ? 1 : 977;
    const float inv = std::ldexp(1.0f, -static_cast<int>(bits - 1));
    uint32_t clipped = 0;
    for (int64_t v = -top; v < top; v += step) CHECK(planarenc::quantise(static_cast<float>(v) * inv, scale, top, &clipped) == v);
    CHECK(planarenc::quantise(static_cast<float>(top - 1) * inv, scale, top, &clipped) == top - 1);
    CHECK(clipped == 0);
  }
}

int main() {
  test_rows();
  test_packed();
  test_quantise();
  if (failures) return 1;
  std::printf("stream_planar_encode_core OK\n");
  return 0;
}
