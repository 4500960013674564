// variable_block_core.h -- the arithmetic of the block-size search (variable_block.cpp), shared by the device kernels
// and a host build (variable_block_cpu.cpp, compiled by g++ for the CPU tests):
//   the coded number of RFC 9639 section 9.1.5 up to 36 bits (the 7-byte UTF-8-like code),
//   a variable-blocking header rewritten from the fixed-blocking header the frame packer wrote,
//   the CRC-16 of the rewritten frame from the old one without reading the body again,
//   the tree minimum over a superblock's dyadic tilings.
#ifndef VARIABLE_BLOCK_CORE_H_
#define VARIABLE_BLOCK_CORE_H_

#include <stdint.h>

#include "flac_decode_core.h"

namespace vbs {

constexpr uint32_t MAX_LEVELS = 5;  // tilings into S, S/2, .., S/16: heap nodes 1 .. 31
constexpr uint32_t MAX_NODES = (1u << MAX_LEVELS) - 1u;
constexpr uint32_t MIN_LEAF = 256;  // the smallest block a search may reach
constexpr uint64_t MAX_SAMPLE_NUMBER = 1ull << 36;

// bytes of the coded number (RFC 9639 section 9.1.5): 1 byte below 2^7, then 11, 16, 21, 26, 31 and 36 bits
FD_HD uint32_t coded_number_bytes(uint64_t v) {
  return v < (1ull << 7) ? 1u : v < (1ull << 11) ? 2u : v < (1ull << 16) ? 3u : v < (1ull << 21) ? 4u
         : v < (1ull << 26) ? 5u : v < (1ull << 31) ? 6u : 7u;
}

// writes the code of v (< 2^36) at p, returns its length
FD_HD uint32_t write_coded_number(uint8_t* p, uint64_t v) {
  const uint32_t n = coded_number_bytes(v);
  if (n == 1) {
    p[0] = static_cast<uint8_t>(v);
    return 1;
  }
  for (uint32_t i = n - 1; i >= 1; --i) {
    p[i] = static_cast<uint8_t>(0x80u | (v & 0x3Fu));
    v >>= 6;
  }
  // n leading ones, a zero, then the top bits (7 bytes: 0xFE and no payload bits in the first byte)
  p[0] = static_cast<uint8_t>((0xFF00u >> n) | static_cast<uint32_t>(v));
  return n;
}

FD_HD uint32_t crc8_bytes(const uint8_t* p, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
  }
  return c;
}

FD_HD uint32_t crc16_bytes(const uint8_t* p, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; ++i) {
    c ^= static_cast<uint32_t>(p[i]) << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
  }
  return c;
}

// Bytes of the header the frame packer writes (sync .. CRC-8) from its first bytes: 4 fixed bytes, the coded number
// (its length is in the first byte's leading ones), the block-size / sample-rate bytes the codes call for, CRC-8.
// 0 for a first byte that is no valid start of a coded number.
FD_HD uint32_t header_bytes(const uint8_t* p) {
  const uint32_t first = p[4];
  uint32_t ones = 0;
  while (ones < 8 && ((first >> (7 - ones)) & 1u)) ++ones;
  if (ones == 1 || ones == 8) return 0;
  const uint32_t num = ones == 0 ? 1u : ones;  // (ones = 7: the 7-byte code)
  const uint32_t bs_code = p[2] >> 4, sr_code = p[2] & 0xFu;
  const uint32_t extra = (bs_code == 6 ? 1u : bs_code == 7 ? 2u : 0u) + (sr_code == 12 ? 1u : (sr_code == 13 || sr_code == 14) ? 2u : 0u);
  return 4u + num + extra + 1u;
}

// The variable-blocking header of the same block: `fixed` is a header as the packer writes it (fixed blocking, coded
// frame number); `out` (room for 16 bytes) receives sync 0xFFF9, the same codes, `sample_number`'s code, the same
// extra bytes and a new CRC-8.  Returns its length (4 + 7 + 2 + 2 + 1 at most).
FD_HD uint32_t write_variable_header(const uint8_t* fixed, uint64_t sample_number, uint8_t* out) {
  const uint32_t h_fixed = header_bytes(fixed);
  uint32_t ones = 0;
  while (ones < 8 && ((fixed[4] >> (7 - ones)) & 1u)) ++ones;
  const uint32_t old_num = ones == 0 ? 1u : ones;
  out[0] = fixed[0];
  out[1] = static_cast<uint8_t>(fixed[1] | 1u);
  out[2] = fixed[2];
  out[3] = fixed[3];
  uint32_t k = 4 + write_coded_number(out + 4, sample_number);
  for (uint32_t i = 4 + old_num; i + 1 < h_fixed; ++i) out[k++] = fixed[i];
  out[k] = static_cast<uint8_t>(crc8_bytes(out, k));
  return k + 1;
}

// CRC-16 (init 0, no xor-out) is linear: crc(H || B) = crc(H) * x^(8|B|) + crc(B) mod P.  So for two headers H, H'
// (each with its CRC-8 byte) in front of the same body B:  crc(H' || B) = crc(H || B) ^ (crc(H) ^ crc(H')) * x^(8|B|).
// x_pow = x^(8|B|) mod P.  The device forms it from XPOW8 (x^(8 * 2^j) mod P for every set bit j of |B|) across the lanes
// of a wave; crc16_rehead is the serial statement.
FD_HD uint32_t crc16_combine(uint32_t crc_old, uint32_t crc_h, uint32_t crc_h_new, uint32_t x_pow) {
  return crc_old ^ flacdec::crc16_mulmod(crc_h ^ crc_h_new, x_pow);
}

struct XPow8 {
  uint16_t v[32];  // x^(8 * 2^j) mod P
};
constexpr XPow8 make_xpow8() {
  XPow8 t{};
  uint32_t base = flacdec::crc16_xpow(8);
  for (int j = 0; j < 32; ++j) {
    t.v[j] = static_cast<uint16_t>(base);
    base = flacdec::crc16_mulmod(base, base);
  }
  return t;
}

FD_HD uint32_t crc16_rehead(uint32_t crc_old, uint32_t crc_h, uint32_t crc_h_new, uint64_t body_bytes) {
  // x^(8n) mod P by square-and-multiply on the 64-bit exponent (frames here are far below 2^32 bytes)
  uint32_t r = 1, base = flacdec::crc16_xpow(8);
  uint64_t n = body_bytes;
  while (n) {
    if (n & 1u) r = flacdec::crc16_mulmod(r, base);
    base = flacdec::crc16_mulmod(base, base);
    n >>= 1;
  }
  return crc16_combine(crc_old, crc_h, crc_h_new, r);
}

// Byte length of a packed fixed-blocking frame recoded with variable blocking: the coded frame number goes, the coded
// sample number comes.
FD_HD uint32_t variable_length(uint32_t fixed_len, uint32_t frame_number, uint64_t sample_number) {
  return fixed_len - coded_number_bytes(frame_number) + coded_number_bytes(sample_number);
}

// The tree minimum of one superblock.  len[n] (n = 1 .. 2^levels - 1, heap order: node 1 the superblock, children of n
// are 2n and 2n + 1) is the coded length of node n.  Bottom-up, node n is split exactly when its children's best sum is
// strictly below len[n] (ties keep the larger block).  Returns the best total; *mask gets bit n - 1 for every split node
// n that lies on the chosen tiling's tree (a split below an unsplit node is not chosen and not set), *frames the number
// of blocks of the tiling.
FD_HD uint64_t tree_min(const uint32_t* len, uint32_t levels, uint32_t* mask, uint32_t* frames) {
  uint64_t best[MAX_NODES + 1];
  uint32_t split = 0;
  const uint32_t first_leaf = 1u << (levels - 1);
  for (uint32_t n = (1u << levels) - 1; n >= 1; --n) {
    best[n] = len[n];
    if (n < first_leaf) {
      const uint64_t kids = best[2 * n] + best[2 * n + 1];
      if (kids < best[n]) {
        best[n] = kids;
        split |= 1u << (n - 1);
      }
    }
  }
  // keep only the splits reachable from the root, count the leaves of the tiling
  uint32_t chosen = 0, count = 0;
  uint32_t stack[MAX_LEVELS + 1];
  uint32_t top = 0;
  stack[top++] = 1;
  while (top) {
    const uint32_t n = stack[--top];
    if (n < first_leaf && ((split >> (n - 1)) & 1u)) {
      chosen |= 1u << (n - 1);
      stack[top++] = 2 * n + 1;
      stack[top++] = 2 * n;
    } else {
      ++count;
    }
  }
  *mask = chosen;
  *frames = count;
  return best[1];
}

// The t-th block (in sample order) of the tiling `mask` of a superblock of `levels` levels: its heap node.
FD_HD uint32_t tiling_node(uint32_t mask, uint32_t levels, uint32_t t) {
  const uint32_t first_leaf = 1u << (levels - 1);
  uint32_t n = 1;
  for (;;) {
    while (n < first_leaf && ((mask >> (n - 1)) & 1u)) n = 2 * n;
    if (t == 0) return n;
    --t;
    while (n & 1u) n >>= 1;  // up while a right child
    if (n == 0) return 0;    // (t beyond the tiling)
    n += 1;
  }
}

// level (depth) of heap node n and its index inside that level
FD_HD uint32_t node_level(uint32_t n) {
  uint32_t k = 0;
  while ((n >> (k + 1)) != 0) ++k;
  return k;
}

}  // namespace vbs
#endif
