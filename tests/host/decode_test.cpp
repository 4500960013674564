// decode_test.cpp -- flacenc::decode_frames (flacenc_rs_amd/host/flacenc.hpp) on frames the library packs itself:
// stereo frames of sigen audio through encode_stereo_frames + pack_stereo_frames, back to back, decoded and compared
// with the input interleaved; a damaged copy of one frame must come back with its status and no samples.
// Build + run: see tests/test_host_decode.py.
#include <cstdio>
#include <vector>

#include "flacenc.hpp"
#include "flacenc_sigen.h"

int main() {
  const size_t nf = 8, n = 4096, bps = 16;
  std::vector<int32_t> x(nf * 2 * n);
  if (flacenc_sigen_fill_frames(x.data(), nf, 2, n, n, bps, 200.0f, 0.4f, 0.3f, 7, 0, 4) != 0) return 2;
  flacenc::HipContext gpu(0);
  flacenc_hip_qlpc_config q{};
  q.lpc_order = 8;
  q.quant_precision = 15;
  q.window_type = FLACENC_HIP_WINDOW_TUKEY;
  q.tukey_alpha = 0.4f;
  q.max_rice_parameter = 30;
  flacenc_hip_frame_config cfg{};
  cfg.qlpc = q;
  cfg.use_constant = cfg.use_lpc = cfg.use_leftside = cfg.use_rightside = cfg.use_midside = 1;
  std::vector<flacenc_hip_stereo_frame_result> res(nf);
  std::vector<int32_t> resid(nf * 2 * n);
  if (flacenc_hip_encode_stereo_frames(gpu.get(), &cfg, x.data(), nf, n, n, bps, res.data(), resid.data(), n,
                                       FLACENC_HIP_MEM_HOST) != 0)
    return 3;
  const size_t stride = (flacenc_hip_stereo_frame_bytes_bound(n, bps) + 15) / 16 * 16;
  std::vector<uint8_t> packed(nf * stride);
  std::vector<uint32_t> len(nf);
  if (flacenc_hip_pack_stereo_frames(gpu.get(), x.data(), nf, n, n, res.data(), resid.data(), n, bps, 44100, 0, 1,
                                     packed.data(), stride, len.data(), FLACENC_HIP_MEM_HOST) != 0)
    return 4;
  std::vector<uint8_t> stream;
  std::vector<uint64_t> off;
  for (size_t f = 0; f < nf; ++f) {
    off.push_back(stream.size());
    stream.insert(stream.end(), packed.begin() + f * stride, packed.begin() + f * stride + len[f]);
  }
  stream[off[3] + len[3] / 2] ^= 0x01;  // damage frame 3
  const auto dec = flacenc::decode_frames(gpu, stream.data(), stream.size(), off, len, 2, bps, n);
  int failures = 0;
  for (size_t f = 0; f < nf; ++f) {
    if (f == 3) {
      if (!(dec[f].status & FLACENC_HIP_DECODE_FRAME_CRC) || !dec[f].samples.empty()) ++failures;
      continue;
    }
    if (dec[f].status || dec[f].block_size != n || dec[f].number != f) ++failures;
    for (size_t t = 0; t < n && !failures; ++t)
      for (size_t c = 0; c < 2; ++c)
        if (dec[f].samples[t * 2 + c] != x[(f * 2 + c) * n + t]) ++failures;
  }
  std::printf("%s: %zu frames decoded\n", failures ? "FAIL" : "decode_test OK", nf);
  return failures ? 1 : 0;
}
