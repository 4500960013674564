// window_lanes_test.cpp -- the lane-major window table of the fused 4096 kernel (flacenc_rs_amd/csrc/window_lanes_core.h)
// against the time-major weights it is built from.  Stand-alone host program: tests/test_window_lanes_host.py writes the
// library's own weights (flacenc_hip_lpc_window_weights) of each window into a file of 4096 floats, and this program
//   * runs window_lanes::build, the builder get_window_entry runs, into a heap block of exactly kFloats floats (so that the
//     sanitizer build sees any write or read past it),
//   * checks every entry (j, lane, i) bit for bit against w[64 lane - 12 + 4 j + i], 0.0f outside [0, 4096),
//   * replays the kernel's reads -- every lane, the quads at the lane-relative offsets -12, -8, ..., 68 through slot_of --
//     against the padded time-major table (32 zeros, the weights, 16 zeros) the kernel read before,
//   * checks the geometry: 21 slots of 1 KB, index() a bijection onto [0, kFloats), every sample of the block present.
// usage: window_lanes_test FILE...
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "window_lanes_core.h"

namespace wl = flacenc_hip::window_lanes;

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char** argv) {
  long failures = 0, entries = 0, zeros_outside = 0, reads = 0;
  auto fail = [&](const char* what, const char* file, int j, int lane, int i) {
    if (++failures <= 20) std::printf("FAIL %s: %s j %d lane %d i %d\n", what, file, j, lane, i);
  };

  // geometry
  static_assert(wl::kSlots == 21 && wl::kLanes == 64 && wl::kSlotFloats * 4 == 1024, "21 slots of 1 KB");
  static_assert(wl::kFloats == 5376 && wl::kFloats * 4 == 21 * 1024, "21 KB");
  static_assert(wl::slot_of(-12) == 0 && wl::slot_of(-8) == 1 && wl::slot_of(0) == 3 && wl::slot_of(68) == wl::kSlots - 1,
                "slots cover the halo at -12 and the look-ahead at +68");
  {
    std::vector<int> seen(wl::kFloats, 0);
    for (int j = 0; j < wl::kSlots; ++j)
      for (int lane = 0; lane < wl::kLanes; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int ix = wl::index(j, lane, i);
          if (ix < 0 || ix >= wl::kFloats || seen[ix]++) fail("index not a bijection", "-", j, lane, i);
          if (ix != (j * 64 + lane) * 4 + i) fail("index formula", "-", j, lane, i);
          if (wl::sample_of(j, lane, i) != 64 * lane - 12 + 4 * j + i) fail("sample formula", "-", j, lane, i);
        }
  }

  for (int f = 1; f < argc; ++f) {
    std::vector<float> w(wl::kBlock);
    FILE* fp = std::fopen(argv[f], "rb");
    if (!fp || std::fread(w.data(), 4, wl::kBlock, fp) != (size_t)wl::kBlock || std::fgetc(fp) != EOF) {
      std::printf("cannot read 4096 floats from %s\n", argv[f]);
      return 2;
    }
    std::fclose(fp);
    // the time-major table as get_window_entry lays it out
    std::vector<float> padded(32 + wl::kBlock + 16, 0.0f);
    std::memcpy(padded.data() + 32, w.data(), wl::kBlock * 4);

    std::unique_ptr<float[]> table(new float[wl::kFloats]);
    for (int k = 0; k < wl::kFloats; ++k) table[k] = -1.0f;  // (no weight is negative: an entry left unwritten shows)
    wl::build(w.data(), table.get());

    std::vector<int> present(wl::kBlock, 0);
    for (int j = 0; j < wl::kSlots; ++j)
      for (int lane = 0; lane < wl::kLanes; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int t = 64 * lane - 12 + 4 * j + i;
          const float got = table[(j * 64 + lane) * 4 + i];
          ++entries;
          if (t < 0 || t >= wl::kBlock) {
            ++zeros_outside;
            if (bits(got) != 0u) fail("nonzero outside the block", argv[f], j, lane, i);
          } else {
            present[t]++;
            if (bits(got) != bits(w[t])) fail("weight differs", argv[f], j, lane, i);
          }
        }
    for (int t = 0; t < wl::kBlock; ++t)
      if (!present[t]) fail("sample missing from the table", argv[f], t, 0, 0);

    // the kernel's reads
    for (int lane = 0; lane < wl::kLanes; ++lane)
      for (int off = -12; off <= 68; off += 4)
        for (int i = 0; i < 4; ++i) {
          const float got = table[wl::index(wl::slot_of(off), lane, i)];
          const float want = padded[32 + 64 * lane + off + i];
          ++reads;
          if (bits(got) != bits(want)) fail("kernel read differs from the time-major table", argv[f], off, lane, i);
        }
  }
  std::printf("%d windows, %ld entries, %ld zeros outside the block, %ld kernel reads, %ld failures\n", argc - 1, entries,
              zeros_outside, reads, failures);
  return failures ? 1 : 0;
}
