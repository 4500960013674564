// wide_encode_core_test.cpp -- the serial statement of the wide encode path (wide_encode_core.h) on the cases of
// tests/wide_cases.py, built stand-alone under AddressSanitizer and UBSan by tests/test_encode_wide_core_cpu.py.
//   wide_encode_core_test <cases> <frames>
// <cases>: uint32 count, then per case 13 uint32 (channels, block, bits, rate, number, use_constant, use_fixed,
// fixed_max_order, max_rice_parameter, use_leftside, use_rightside, use_midside, wasted_bits) and channels x block int32.
// <frames>: per case uint32 length (0: the writer's own check failed), uint32 bytes bound, the bytes.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "wide_encode_core.h"

namespace {

// the bounds of frame_pack.cpp (flacenc_hip_frame_bytes_bound / _stereo_frame_bytes_bound before rounding to 16)
size_t bytes_bound(uint32_t channels, uint32_t n, uint32_t bits) {
  const size_t body = channels == 2 ? 16 + static_cast<size_t>(n) * (2 * bits + 1) : static_cast<size_t>(channels) * (8 + static_cast<size_t>(n) * bits);
  return 15 + (body + 7) / 8 + 2;
}

bool read_words(FILE* f, void* dst, size_t words) { return fread(dst, 4, words, f) == words; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t count = 0;
  if (!read_words(in, &count, 1)) return 2;
  std::unique_ptr<wideenc::Tables> tab(new wideenc::Tables);
  std::vector<wideenc::SubRecord> recs(8);
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t h[13];
    if (!read_words(in, h, 13)) return 2;
    const uint32_t channels = h[0], n = h[1], bits = h[2];
    if (channels < 1 || channels > 8 || n < 1 || n > 32767 || bits < 8 || bits > 32) return 2;
    std::vector<int32_t> x(static_cast<size_t>(channels) * n);
    if (!read_words(in, x.data(), x.size())) return 2;
    const wideenc::Config c = {h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12]};
    const size_t bound = bytes_bound(channels, n, bits), room = (bound + 15) & ~static_cast<size_t>(15);
    std::vector<uint32_t> frame(room / 4);  // exactly the slot the library asks for: ASan guards its end
    const wideenc::Rows rows = {x.data(), n, channels};
    const uint32_t len = wideenc::write_frame(rows, n, bits, h[3], h[4], c, tab.get(), recs.data(),
                                              reinterpret_cast<uint8_t*>(frame.data()), room);
    const uint32_t head[2] = {len, static_cast<uint32_t>(bound)};
    fwrite(head, 4, 2, out);
    fwrite(frame.data(), 1, len, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("wide OK %u\n", count);
  return 0;
}
