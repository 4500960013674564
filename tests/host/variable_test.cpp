// variable_test.cpp -- HipContext::encode_variable (flacenc_rs_amd/host/flacenc.hpp): stereo sigen audio coded with
// the block-size search, its frames decoded back by flacenc::decode_frames and compared with the input.
// Build + run: see tests/test_host_variable.py.
#include <cstdio>
#include <vector>

#include "flacenc.hpp"
#include "flacenc_sigen.h"

int main() {
  const size_t nsb = 6, n = 4096, bps = 16, levels = 3;
  const uint64_t total = nsb * n - 1000, first = 123456;
  std::vector<int32_t> x(nsb * 2 * n);
  if (flacenc_sigen_fill_frames(x.data(), nsb, 2, n, n, bps, 200.0f, 0.4f, 0.3f, 11, 0, 4) != 0) return 2;
  for (size_t c = 0; c < 2; ++c)  // zero beyond total_samples, as fill_le_bytes leaves the last superblock
    for (size_t t = total % n; t < n; ++t) x[((nsb - 1) * 2 + c) * n + t] = 0;
  flacenc::HipContext gpu(0);
  flacenc_hip_frame_config cfg{};
  cfg.qlpc.lpc_order = 8;
  cfg.qlpc.quant_precision = 15;
  cfg.qlpc.window_type = FLACENC_HIP_WINDOW_TUKEY;
  cfg.qlpc.tukey_alpha = 0.4f;
  cfg.qlpc.max_rice_parameter = 30;
  cfg.use_constant = cfg.use_lpc = cfg.use_leftside = cfg.use_rightside = cfg.use_midside = 1;
  const flacenc::VariableFrames v = gpu.encode_variable(cfg, x.data(), total, 2, n, levels, bps, 44100, first);
  const std::vector<flacenc::DecodedFrame> d =
      flacenc::decode_frames(gpu, v.bytes.data(), v.bytes.size(), v.offsets, v.lengths, 2, bps, n);
  uint64_t pos = 0;
  for (size_t f = 0; f < d.size(); ++f) {
    if (d[f].status != 0 || d[f].block_size != v.block_sizes[f] || d[f].number != first + pos) {
      std::printf("frame %zu: status %u block %zu number %llu\n", f, d[f].status, d[f].block_size,
                  static_cast<unsigned long long>(d[f].number));
      return 4;
    }
    for (size_t t = 0; t < d[f].block_size; ++t)
      for (size_t c = 0; c < 2; ++c) {
        const uint64_t s = pos + t;
        if (d[f].samples[t * 2 + c] != x[((s / n) * 2 + c) * n + s % n]) return 5;
      }
    pos += d[f].block_size;
  }
  if (pos != total) return 6;
  std::printf("variable_test OK: %zu frames, %zu bytes\n", d.size(), v.bytes.size());
  return 0;
}
