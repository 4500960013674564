// variable_block_cpu.cpp -- the host build of variable_block_core.h (g++): a C interface for the CPU tests
// (flacenc_rs_amd/variable_cpu.py) and, with -DVBS_MAIN, a self-checking driver the tests run under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "variable_block_core.h"

namespace {
const flacdec::CrcTables kTab = flacdec::make_crc_tables();
}

extern "C" {

uint32_t vbs_coded_number_bytes(uint64_t v) { return vbs::coded_number_bytes(v); }
uint32_t vbs_write_coded_number(uint8_t* p, uint64_t v) { return vbs::write_coded_number(p, v); }
uint32_t vbs_header_bytes(const uint8_t* p) { return vbs::header_bytes(p); }
uint32_t vbs_write_variable_header(const uint8_t* fixed, uint64_t sample_number, uint8_t* out) {
  return vbs::write_variable_header(fixed, sample_number, out);
}
uint32_t vbs_crc16(const uint8_t* p, uint64_t n) {
  uint32_t c = 0;
  for (uint64_t i = 0; i < n; ++i) c = ((c << 8) & 0xFFFFu) ^ kTab.t16[((c >> 8) ^ p[i]) & 0xFFu];
  return c;
}
uint32_t vbs_crc16_rehead(uint32_t crc_old, uint32_t crc_h, uint32_t crc_h_new, uint64_t body_bytes) {
  return vbs::crc16_rehead(crc_old, crc_h, crc_h_new, body_bytes);
}
uint64_t vbs_tree_min(const uint32_t* len, uint32_t levels, uint32_t* mask, uint32_t* frames) {
  return vbs::tree_min(len, levels, mask, frames);
}
uint32_t vbs_tiling_node(uint32_t mask, uint32_t levels, uint32_t t) { return vbs::tiling_node(mask, levels, t); }
// flacdec::parse_header on len bytes: status; out = block_size, channels, bps, header_bytes, variable; *number
uint32_t vbs_parse_header(const uint8_t* p, uint32_t len, uint32_t channels, uint32_t bits_per_sample,
                          uint32_t* out, uint64_t* number) {
  flacdec::Header h{};
  const uint32_t st = flacdec::parse_header(p, len, channels, bits_per_sample, 65536, flacdec::MAX_BPS, kTab, h);
  out[0] = h.block_size;
  out[1] = h.channels;
  out[2] = h.bps;
  out[3] = h.header_bytes;
  out[4] = h.variable;
  *number = h.number;
  return st;
}

}  // extern "C"

#ifdef VBS_MAIN
// Self-check of the core on its own: run under the sanitizers by the CPU tests.  Exit status 0 = all passed.
namespace {
int failures = 0;
void check(bool ok, const char* what, uint64_t a, uint64_t b) {
  if (!ok && failures++ < 20) fprintf(stderr, "FAIL %s: %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b);
}

// a fixed-blocking header as the packer writes it: codes, frame number, extra bytes, CRC-8
uint32_t fixed_header(uint8_t* p, uint32_t frame_number, uint32_t bs_code, uint32_t sr_code, std::mt19937_64& rng) {
  p[0] = 0xFF;
  p[1] = 0xF8;
  p[2] = static_cast<uint8_t>((bs_code << 4) | sr_code);
  p[3] = static_cast<uint8_t>((1u << 4) | (4u << 1));
  uint32_t k = 4 + vbs::write_coded_number(p + 4, frame_number);
  const uint32_t extra = (bs_code == 6 ? 1u : bs_code == 7 ? 2u : 0u) + (sr_code == 12 ? 1u : (sr_code == 13 || sr_code == 14) ? 2u : 0u);
  for (uint32_t i = 0; i < extra; ++i) p[k++] = static_cast<uint8_t>(rng());
  p[k] = static_cast<uint8_t>(vbs::crc8_bytes(p, k));
  return k + 1;
}
}  // namespace

int main() {
  std::mt19937_64 rng(0x5EEDB10Cull);
  // coded numbers round-trip through the decoder's header parser at every 2^k boundary up to 2^36
  for (uint32_t k = 0; k <= 36; ++k) {
    for (int64_t d = -1; d <= 1; ++d) {
      const int64_t v = (int64_t(1) << k) + d;
      if (v < 0 || uint64_t(v) >= vbs::MAX_SAMPLE_NUMBER) continue;
      uint8_t fixed[16], var[16];
      const uint32_t hf = fixed_header(fixed, 1, 12, 9, rng);
      check(vbs::header_bytes(fixed) == hf, "fixed header length", vbs::header_bytes(fixed), hf);
      const uint32_t hv = vbs::write_variable_header(fixed, uint64_t(v), var);
      check(hv == hf - 1 + vbs::coded_number_bytes(uint64_t(v)), "variable header length", hv, hf);
      flacdec::Header h{};
      const uint32_t st = flacdec::parse_header(var, hv, 2, 16, 65536, flacdec::MAX_BPS, kTab, h);
      check(st == 0 && h.variable == 1 && h.number == uint64_t(v) && h.header_bytes == hv && h.block_size == 4096,
            "parse_header of the variable header", h.number, uint64_t(v));
    }
  }
  // the CRC-16 combine equals a direct CRC on random frames and header pairs
  for (int trial = 0; trial < 200; ++trial) {
    const uint32_t body = trial < 8 ? trial : static_cast<uint32_t>(rng() % (trial < 190 ? 70000 : (1u << 20)));
    std::vector<uint8_t> b(body);
    for (auto& x : b) x = static_cast<uint8_t>(rng());
    const uint32_t codes[4][2] = {{12, 9}, {6, 12}, {7, 13}, {11, 14}};
    const uint32_t* c = codes[trial % 4];
    uint8_t fixed[16], var[16];
    const uint32_t fn = static_cast<uint32_t>(rng() % (1ull << (rng() % 31 + 1)));
    const uint32_t hf = fixed_header(fixed, fn, c[0], c[1], rng);
    const uint64_t sample = rng() % vbs::MAX_SAMPLE_NUMBER >> (rng() % 36);
    const uint32_t hv = vbs::write_variable_header(fixed, sample, var);
    std::vector<uint8_t> f1(fixed, fixed + hf), f2(var, var + hv);
    f1.insert(f1.end(), b.begin(), b.end());
    f2.insert(f2.end(), b.begin(), b.end());
    const uint32_t old = vbs_crc16(f1.data(), f1.size()), want = vbs_crc16(f2.data(), f2.size());
    const uint32_t got = vbs::crc16_rehead(old, vbs::crc16_bytes(fixed, hf), vbs::crc16_bytes(var, hv), body);
    check(got == want, "crc16 combine", got, want);
    // the device's form of x^(8|B|): the product of XPOW8 over |B|'s set bits
    constexpr vbs::XPow8 xp = vbs::make_xpow8();
    uint32_t p = 1;
    for (int j = 0; j < 32; ++j)
      if ((body >> j) & 1u) p = flacdec::crc16_mulmod(p, xp.v[j]);
    const uint32_t got2 = vbs::crc16_combine(old, vbs::crc16_bytes(fixed, hf), vbs::crc16_bytes(var, hv), p);
    check(got2 == want, "crc16 combine from XPOW8", got2, want);
  }
  // the tree minimum: its total and frame count agree with the tiling its mask describes
  for (int trial = 0; trial < 5000; ++trial) {
    const uint32_t levels = 1 + trial % vbs::MAX_LEVELS;
    uint32_t len[vbs::MAX_NODES + 1] = {0};
    const uint32_t spread = trial % 3 == 0 ? 3u : 1000u;  // small spreads give ties
    for (uint32_t n = 1; n < (1u << levels); ++n) len[n] = static_cast<uint32_t>(100u * (levels - vbs::node_level(n)) + rng() % spread);
    uint32_t mask = 0, frames = 0;
    const uint64_t best = vbs::tree_min(len, levels, &mask, &frames);
    // recompute the total and frame count from the mask's tiling
    uint64_t sum = 0;
    uint32_t count = 0;
    for (uint32_t t = 0;; ++t) {
      const uint32_t n = vbs::tiling_node(mask, levels, t);
      if (n == 0) break;
      sum += len[n];
      ++count;
    }
    check(sum == best && count == frames, "tiling of the mask", sum, best);
  }
  printf("variable_block_core self-check: %d failures\n", failures);
  return failures ? 1 : 0;
}
#endif
