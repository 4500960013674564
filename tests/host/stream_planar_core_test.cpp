// stream_planar_core_test.cpp -- csrc/stream_planar_core.h against brute force, as a stand-alone program for the address
// and undefined-behaviour sanitizers (tests/test_decode_ranges_planar_cpu.py builds and runs it):
//   the slot: channels 1..8, n_samples 0..40 -- every element's address, computed by walking the slot element by
//     element, lies inside the slot, and every 4-byte cell of the slot belongs to exactly one element
//   the split: a writer that stores head, body and tail as the kernels do (scalars, whole 16-byte vectors at 16-byte
//     aligned addresses only, scalars) into a guarded buffer touches exactly the interval, for every row start
//     (channel, n_samples, slot offset 0 / 4 / 8 / 12 mod 16), every destination and every count that fits the row --
//     so every way the three parts can move across a 16-byte boundary
//   the zero interval, the value rule at the ends of the 8-, 16- and 24-bit ranges and on values that do not fit, and
//     the check of the range table
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_planar_core.h"

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

static void test_slot_and_addresses() {
  for (uint32_t channels = 1; channels <= 8; ++channels)
    for (uint64_t n = 0; n <= 40; ++n)
      for (uint64_t slot = 0; slot <= 12; slot += 4) {
        const uint64_t bytes = streamplanar::slot_bytes(channels, n);
        CHECK(bytes == channels * n * 4);
        std::vector<int> owner(bytes / 4, 0);
        uint64_t walk = slot;  // element after element, row after row
        for (uint32_t c = 0; c < channels; ++c)
          for (uint64_t i = 0; i < n; ++i, walk += 4) {
            const uint64_t at = streamplanar::element_offset(slot, n, c, i);
            CHECK(at == walk && at % 4 == 0 && at >= slot && at + 4 <= slot + bytes);
            if (at >= slot && at + 4 <= slot + bytes) ++owner[(at - slot) / 4];
          }
        for (int v : owner) CHECK(v == 1);
      }
}

// what the kernels do with a split: `count` elements of value `mark` from element `first` of a buffer whose element 0
// lies at byte address `base` (a multiple of 4): returns false when a vector store would be misaligned
static bool store_split(std::vector<uint32_t>& cells, uint64_t base, uint64_t first, uint64_t count, uint32_t mark) {
  const uint64_t addr = base + first * 4;
  const streamplanar::Split s = streamplanar::split(addr, count);
  if (s.head + s.body + s.tail != count || s.head > 3 || s.tail > 3 || s.body % 4) return false;
  // the head ends at a 16-byte boundary unless the interval does before it
  if (s.body && (addr + 4 * s.head) % 16) return false;
  if (s.head < count && (addr + 4 * s.head) % 16) return false;
  uint64_t at = first;
  for (uint32_t k = 0; k < s.head; ++k) cells.at(at++) = mark;
  for (uint64_t v = 0; v < s.body; v += 4) {
    if ((base + at * 4) % 16) return false;
    for (int k = 0; k < 4; ++k) cells.at(at++) = mark;
  }
  for (uint32_t k = 0; k < s.tail; ++k) cells.at(at++) = mark;
  return at == first + count;
}

static void test_split() {
  const uint32_t FILL = 0xA5A5A5A5u, MARK = 0x1234ABCDu;
  for (uint32_t channels = 1; channels <= 8; ++channels)
    for (uint64_t n = 0; n <= 40; ++n)
      for (uint64_t slot = 64; slot <= 76; slot += 4)
        for (uint32_t c = 0; c < channels; ++c) {
          // the row of channel c between four guard cells on either side; every interval [dst, dst + take) of it, the
          // writer's and the zero pass's alike
          const uint64_t row = streamplanar::element_offset(slot, n, c, 0);
          std::vector<uint32_t> cells(n + 8);
          for (uint64_t dst = 0; dst <= n; ++dst)
            for (uint64_t take = 0; dst + take <= n; ++take) {
              cells.assign(n + 8, FILL);
              CHECK(streamplanar::element_offset(slot, n, c, dst) == row + 4 * dst);
              CHECK(store_split(cells, row - 16, 4 + dst, take, MARK));
              for (uint64_t i = 0; i < n + 8; ++i) CHECK(cells[i] == (i >= 4 + dst && i < 4 + dst + take ? MARK : FILL));
            }
        }
  // every residue and every count around the boundaries, with the parts spelled out
  for (uint64_t addr = 0; addr < 64; addr += 4)
    for (uint64_t count = 0; count <= 40; ++count) {
      const streamplanar::Split s = streamplanar::split(addr, count);
      uint64_t head = 0;
      while (head < count && (addr + 4 * head) % 16) ++head;
      CHECK(s.head == head);
      CHECK(s.body == (count - head) / 4 * 4);
      CHECK(s.tail == (count - head) % 4);
      const uint32_t lead = streamplanar::lead(addr);
      CHECK(lead == addr % 16 / 4 && (addr - 4 * lead) % 16 == 0);
      CHECK(s.head == (count < ((4 - lead) & 3) ? count : (4 - lead) & 3));
    }
  // the decoder's writer: elements staged where they lie behind the 16-byte boundary in front of the row (`lead` words
  // that are not the lane's first), flushed at arbitrary moments (here: whenever `every` more have been staged) and at
  // the end -- whole vectors from the first boundary on, the head and what is left one by one
  for (uint64_t addr = 64; addr < 80; addr += 4)
    for (uint64_t count = 0; count <= 40; ++count)
      for (uint32_t every = 1; every <= 16; ++every) {
        std::vector<uint32_t> cells(count + 12, FILL);  // cell i at byte 48 + 4 i: four guard cells in front at least
        const uint64_t first = (addr - 48) / 4;
        uint32_t stage[20];
        uint32_t lead = streamplanar::lead(addr), fill = lead;
        uint64_t to = first - lead;  // the cell stage[0] belongs to, 16-byte aligned
        CHECK((48 + 4 * to) % 16 == 0);
        auto flush = [&]() {
          const uint32_t vectors = fill / 4;
          if (!vectors) return;
          for (uint32_t g = 0; g < vectors; ++g)
            for (uint32_t k = (g == 0 ? lead : 0); k < 4; ++k) cells.at(to + 4 * g + k) = stage[4 * g + k];
          for (uint32_t k = 0; k < fill % 4; ++k) stage[k] = stage[4 * vectors + k];
          to += 4 * vectors;
          lead = 0;
          fill %= 4;
        };
        for (uint64_t i = 0; i < count; ++i) {
          CHECK(fill < 20);
          stage[fill++] = MARK + static_cast<uint32_t>(i);
          if ((i + 1) % every == 0) flush();
        }
        flush();
        for (uint32_t k = lead; k < fill; ++k) cells.at(to + k) = stage[k];
        for (uint64_t i = 0; i < cells.size(); ++i)
          CHECK(cells[i] == (i >= first && i < first + count ? MARK + static_cast<uint32_t>(i - first) : FILL));
      }
  // large addresses and counts
  const streamplanar::Split big = streamplanar::split(0xFFFFFFFFFFF4ull, (1ull << 40) + 6);
  CHECK(big.head == 3 && big.body == (1ull << 40) && big.tail == 3);
}

static void test_zero_interval() {
  for (uint64_t n = 0; n <= 40; ++n)
    for (uint64_t w = 0; w <= n; ++w) {
      const streamplanar::Interval z = streamplanar::zero_interval(w, n);
      CHECK(z.first == w && z.count == n - w);
      std::vector<int> row(n, 1);
      for (uint64_t i = z.first; i < z.first + z.count; ++i) row.at(i) = 0;
      for (uint64_t i = 0; i < n; ++i) CHECK(row[i] == (i < w ? 1 : 0));
    }
  const streamplanar::Interval none = streamplanar::zero_interval(0, 0);
  CHECK(none.count == 0);
  const streamplanar::Interval huge = streamplanar::zero_interval(0, ~0ull);
  CHECK(huge.first == 0 && huge.count == ~0ull);
}

static float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static void test_values() {
  for (uint32_t bits = 4; bits <= 24; ++bits) {
    const float scale = streamplanar::scale_of(bits);
    CHECK(scale == std::ldexp(1.0f, -static_cast<int>(bits - 1)));
    const int32_t lo = -(1 << (bits - 1)), hi = (1 << (bits - 1)) - 1;
    CHECK(as_float(streamplanar::element(lo, FLACENC_HIP_SAMPLE_F32, scale)) == -1.0f);
    CHECK(as_float(streamplanar::element(hi, FLACENC_HIP_SAMPLE_F32, scale)) == 1.0f - std::ldexp(1.0f, -static_cast<int>(bits - 1)));
    CHECK(streamplanar::element(0, FLACENC_HIP_SAMPLE_F32, scale) == 0u);  // +0.0f
    CHECK(streamplanar::element(lo, FLACENC_HIP_SAMPLE_I32, scale) == static_cast<uint32_t>(lo));
    // every value of the depth is exact: value == element * 2^(bits - 1)
    for (int32_t v = lo; v <= hi; v += (bits > 12 ? 257 : 1))
      CHECK(std::ldexp(as_float(streamplanar::element(v, FLACENC_HIP_SAMPLE_F32, scale)), bits - 1) == static_cast<float>(v) &&
            static_cast<int32_t>(static_cast<float>(v)) == v);
  }
  // values that do not fit 24 bits round to nearest even on the way to float, then scale exactly
  const float s16 = streamplanar::scale_of(16);
  CHECK(as_float(streamplanar::element(0x7FFFFFFF, FLACENC_HIP_SAMPLE_F32, s16)) == 65536.0f);
  CHECK(as_float(streamplanar::element(INT32_MIN, FLACENC_HIP_SAMPLE_F32, s16)) == -65536.0f);
  CHECK(as_float(streamplanar::element((1 << 24) + 1, FLACENC_HIP_SAMPLE_F32, s16)) == 512.0f);       // ties to even
  CHECK(as_float(streamplanar::element((1 << 24) + 3, FLACENC_HIP_SAMPLE_F32, s16)) == 512.0f + 4.0f / 32768.0f);
  CHECK(streamplanar::element(0x7FFFFFFF, FLACENC_HIP_SAMPLE_I32, s16) == 0x7FFFFFFFu);
}

static Desc desc(uint32_t channels, uint32_t width) {
  Desc d{};
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
  std::vector<Desc> t{desc(2, 2), desc(1, 3), desc(8, 4)};
  auto one = [&](Range r, uint64_t out_bytes) { return streamplanar::check_ranges(&r, 1, t.data(), t.size(), out_bytes); };
  CHECK(one(range(0, 10, 0, 0), 80) == FLACENC_HIP_OK);                        // 2 * 10 * 4 bytes, whatever the width
  CHECK(one(range(0, 10, 4, 0), 80) == FLACENC_HIP_ERR_BAD_ARGUMENT);          // four bytes past
  CHECK(one(range(0, 10, 0, 0), 79) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 10, 0, 1), 40) == FLACENC_HIP_OK);                        // 3-byte samples take 4 bytes too
  CHECK(one(range(0, 10, 0, 1), 39) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  for (uint64_t off = 1; off < 16; ++off)
    CHECK(one(range(0, 1, off, 1), 400) == (off % 4 ? FLACENC_HIP_ERR_BAD_ARGUMENT : FLACENC_HIP_OK));
  CHECK(one(range(0, 0, 2, 1), 400) == FLACENC_HIP_ERR_BAD_ARGUMENT);          // an empty slot is aligned too
  CHECK(one(range(5, 0, 40, 1), 40) == FLACENC_HIP_OK);                        // an empty slot at the very end
  CHECK(one(range(5, 0, 44, 1), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 1, 8, 2), 40) == FLACENC_HIP_OK);                         // 32 bytes a sample
  CHECK(one(range(0, 1, 12, 2), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 1, 0, 3), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);           // no such stream
  CHECK(one(range(0, 1, 0, 0, 1), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);        // reserved
  CHECK(one(range(~0ull, 1, 0, 0), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);       // first + n wraps
  CHECK(one(range(0, ~0ull, 0, 0), ~0ull) == FLACENC_HIP_ERR_BAD_ARGUMENT);    // n * 8 wraps
  CHECK(one(range(0, (1ull << 61) + 1, 0, 0), ~0ull) == FLACENC_HIP_ERR_BAD_ARGUMENT);
  CHECK(one(range(0, 1, ~0ull - 3, 0), 40) == FLACENC_HIP_ERR_BAD_ARGUMENT);   // a multiple of 4 far past the end
  CHECK(streamplanar::check_ranges(nullptr, 0, t.data(), t.size(), 0) == FLACENC_HIP_OK);
}

int main() {
  test_slot_and_addresses();
  test_split();
  test_zero_interval();
  test_values();
  test_checks();
  if (failures) return 1;
  std::printf("stream_planar_core OK\n");
  return 0;
}
