// stream_recover_core_test.cpp -- csrc/stream_recover_core.h against brute force on random small chains, 64-bit
// extremes included.  A stand-alone program (tests/test_recover_core_cpu.py builds it with -fsanitize=address,undefined):
//   coded_position / scan_value   against the rule's words
//   combine                       associative; the segmented inclusive scan built from it in blocks of any size (the
//                                 shape of the three-launch device scan) equals the serial per-stream maximum
//   is_placed                     with the scan's prefix maximum equals the serial rule
//   cut_frames                    equals the first placed frame that no longer fits, found by a loop
//   gap_before, pieces_of         the gaps of the written frames tile [0, L) together with the frames
//   zero_split                    head + 16 * vectors + tail is the range, vectors start and end on 16-byte boundaries
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "stream_recover_core.h"

using namespace streamrecover;

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      printf("FAILED %s (line %d)\n", #c, __LINE__);         \
      exit(1);                                               \
    }                                                        \
  } while (0)

struct F {
  uint64_t number;
  uint32_t variable, block;
};

int main() {
  std::mt19937_64 rng(0x5EC0FE);
  // ---- positions
  CHECK(coded_position(7, 0, 4096) == 7ull * 4096);
  CHECK(coded_position(7, 1, 4096) == 7);
  CHECK(coded_position((1ull << 36) - 1, 0, 65536) == ((1ull << 36) - 1) * 65536);  // the largest: below 2^52
  CHECK(coded_position((1ull << 36) - 1, 1, 1) == (1ull << 36) - 1);
  CHECK(scan_value(10, 5, 0) == 15 && scan_value(10, 5, 100) == 100 && scan_value(10, 5, 15) == 15);
  CHECK(scan_value(((1ull << 36) - 1) * 65536, 65536, ~0ull) == ~0ull);

  // ---- zero_split
  for (uint64_t lo = 0; lo < 70; ++lo)
    for (uint64_t hi = lo; hi < lo + 80; ++hi) {
      for (uint64_t shift : {0ull, 4096ull, (1ull << 47) - 32}) {
        const ZeroSplit z = zero_split(lo + shift, hi + shift);
        CHECK(z.head + 16 * z.vectors + z.tail == hi - lo);
        CHECK(z.head < 16 || z.vectors == 0);
        CHECK(z.tail < 16);
        if (z.vectors) CHECK((lo + shift + z.head) % 16 == 0);
        if (z.vectors == 0 && z.tail) CHECK((lo + shift + z.head) % 16 == 0);
        if (hi - lo >= 31) CHECK(z.vectors >= 1);
      }
    }
  CHECK(pieces_of(0) == 0 && pieces_of(1) == 1 && pieces_of(PIECE) == 1 && pieces_of(PIECE + 1) == 2);

  // ---- chains
  for (int round = 0; round < 4000; ++round) {
    const uint32_t n_streams = 1 + rng() % 5;
    const bool extreme = round % 7 == 0;
    std::vector<uint64_t> base(n_streams + 1, 0), origin(n_streams);
    std::vector<uint32_t> mbs(n_streams), width(n_streams);
    std::vector<uint64_t> capacity(n_streams);
    std::vector<F> frames;
    std::vector<uint32_t> owner;
    for (uint32_t s = 0; s < n_streams; ++s) {
      const uint32_t count = rng() % 9;
      mbs[s] = extreme ? 65536 : 16 + rng() % 48;
      width[s] = 1 + rng() % 32;
      const uint32_t variable = rng() % 2;
      origin[s] = rng() % 3 ? 0 : (extreme ? (rng() % 2 ? ~0ull : (1ull << 51)) : rng() % 200);
      uint64_t at = variable ? origin[s] : origin[s] / mbs[s];
      for (uint32_t k = 0; k < count; ++k) {
        F f;
        f.variable = variable;
        f.block = extreme ? 1 + rng() % 65536 : 1 + rng() % (mbs[s] + 8);
        const uint32_t what = rng() % 8;
        if (what == 0) at = rng() % (at + 2);                                  // jumps back
        if (what == 1) at += rng() % 5;                                        // a hole
        if (extreme && what == 2) at = (1ull << 36) - 1 - rng() % 3;           // the largest numbers
        f.number = at & ((1ull << 36) - 1);
        frames.push_back(f);
        owner.push_back(s);
        at = f.number + (variable ? f.block : 1);
      }
      base[s + 1] = frames.size();
      capacity[s] = rng() % 4 == 0 ? rng() % 50 : (extreme ? rng() : rng() % 40000);
    }
    const size_t n = frames.size();
    // the device's shape: blocks of B elements, aggregates, exclusive combination, apply
    std::vector<uint64_t> P(n), V(n), emax(n);
    std::vector<SegMax> el(n);
    for (size_t m = 0; m < n; ++m) {
      const uint32_t s = owner[m];
      P[m] = coded_position(frames[m].number, frames[m].variable, mbs[s]);
      V[m] = scan_value(P[m], frames[m].block, origin[s]);
      el[m] = SegMax{m == base[s] ? 1u : 0u, V[m]};
    }
    const size_t B = 1 + rng() % 6;
    std::vector<SegMax> agg;
    for (size_t b = 0; b * B < n; ++b) {
      SegMax a{0, 0};
      for (size_t m = b * B; m < n && m < (b + 1) * B; ++m) a = combine(a, el[m]);
      agg.push_back(a);
    }
    SegMax carry{0, 0};
    for (size_t b = 0; b < agg.size(); ++b) {
      SegMax a = carry;
      for (size_t m = b * B; m < n && m < (b + 1) * B; ++m) {
        a = combine(a, el[m]);
        emax[m] = a.v;
      }
      carry = combine(carry, agg[b]);
      CHECK(a.head == carry.head && a.v == carry.v);  // associativity, block by block
    }
    if (n >= 3) {
      const size_t i = rng() % (n - 2);
      const SegMax l = combine(combine(el[i], el[i + 1]), el[i + 2]), r = combine(el[i], combine(el[i + 1], el[i + 2]));
      CHECK(l.head == r.head && l.v == r.v);
    }
    for (uint32_t s = 0; s < n_streams; ++s) {
      const uint64_t first = base[s], count = base[s + 1] - first, W = width[s];
      // brute force: the serial rule
      uint64_t top = origin[s];
      std::vector<char> placed(count);
      for (uint64_t k = 0; k < count; ++k) {
        const F& f = frames[first + k];
        const uint64_t p = f.variable ? f.number : f.number * mbs[s], e = p + f.block;
        CHECK(p == P[first + k]);
        placed[k] = f.block <= mbs[s] && p >= origin[s] && p >= top;
        CHECK(placed[k] == is_placed(p, f.block, mbs[s], origin[s], k ? emax[first + k - 1] : origin[s]));
        if (e > top) top = e;
        CHECK(emax[first + k] == top);
        if (placed[k]) CHECK(emax[first + k] == e);
      }
      // the cut: written = the placed frames in front of the first placed one that does not fit
      uint64_t written = 0, L = 0, covered = 0, prev_end = origin[s], pieces = 0;
      bool no_room = false;
      std::vector<char> is_written(count, 0);
      for (uint64_t k = 0; k < count && !no_room; ++k) {
        if (!placed[k]) continue;
        const unsigned __int128 need = static_cast<unsigned __int128>(P[first + k] + frames[first + k].block - origin[s]) * W;
        if (need > capacity[s]) {
          no_room = true;
          break;
        }
        is_written[k] = 1;
        ++written;
      }
      const uint64_t cut = cut_frames(emax.data(), first, count, origin[s], static_cast<uint32_t>(W), capacity[s]);
      uint64_t got = 0;
      bool placed_behind = false;
      for (uint64_t k = 0; k < count; ++k) {
        if (placed[k] && k < cut) {
          CHECK(is_written[k]);
          ++got;
        }
        if (placed[k] && k >= cut) placed_behind = true;
      }
      CHECK(got == written && placed_behind == no_room);
      // gaps and frames tile [0, L)
      for (uint64_t k = 0; k < count; ++k) {
        if (!is_written[k]) continue;
        const uint64_t g = gap_before(P[first + k], prev_end);
        CHECK(P[first + k] >= prev_end);
        covered += g + frames[first + k].block;
        pieces += pieces_of(g * W);
        prev_end = P[first + k] + frames[first + k].block;
        L = prev_end - origin[s];
      }
      CHECK(covered == L);
      CHECK(static_cast<unsigned __int128>(L) * W <= capacity[s]);
      (void)pieces;
    }
  }
  printf("stream_recover_core OK\n");
  return 0;
}
