// md5_core.h -- the arithmetic of RFC 1321, shared by the device kernel (md5_streams.cpp: one lane per span) and its
// host test (tests/host/md5_core_test.cpp, compiled by g++ for the CPU tests).  No HIP types.
//
//   md5_init()        the initial state A, B, C, D
//   md5_block()       one 64-byte block, given as 16 little-endian words, into the state.  The 64 steps are written out:
//                     every m[g] index and every additive constant is a compile-time constant, so on the device the
//                     message words stay in registers (a runtime-indexed m[] would move them to scratch)
//   md5_pad_word()    word j of a block of the message's end: data bytes while there are any, then 0x80, zeros, and in
//                     the last block the bit length -- the FULL 64-bit value 8 * total.  The bytes come through
//                     `byte_at(i)`, which is called for i < total only: nothing behind the message is ever read
//   md5_pad_blocks()  the one or two padded blocks behind the whole blocks, from the at most 63 bytes they leave
//   md5_digest()      the state as the 16 digest bytes: A, B, C, D, each little-endian -- what hashlib.md5(x).digest()
//                     returns and what STREAMINFO stores
//   md5_bytes()       all of it for one byte string on the host
//
// One stream alone is hashed faster by one host core than by one lane; the device form exists for batches of spans.
#ifndef MD5_CORE_H_
#define MD5_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define MD5_HD __host__ __device__ inline
#else
#define MD5_HD inline
#endif

namespace md5core {

MD5_HD void md5_init(uint32_t state[4]) {
  state[0] = 0x67452301u;
  state[1] = 0xefcdab89u;
  state[2] = 0x98badcfeu;
  state[3] = 0x10325476u;
}

// rotate left by a constant 1..31: the builtin where the compiler has it (clang, so the device: one v_alignbit_b32)
MD5_HD uint32_t md5_rotl(uint32_t x, uint32_t s) {
#if defined(__clang__)
  return __builtin_rotateleft32(x, s);
#else
  return (x << s) | (x >> (32u - s));
#endif
}

#define MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, g, s, t)                   \
  do {                                                     \
    (a) += f((b), (c), (d)) + m[g] + static_cast<uint32_t>(t); \
    (a) = md5_rotl((a), (s)) + (b);                            \
  } while (0)

MD5_HD void md5_block(uint32_t state[4], const uint32_t m[16]) {
  uint32_t a = state[0], b = state[1], c = state[2], d = state[3];
  MD5_STEP(MD5_F, a, b, c, d, 0, 7, 0xd76aa478u);
  MD5_STEP(MD5_F, d, a, b, c, 1, 12, 0xe8c7b756u);
  MD5_STEP(MD5_F, c, d, a, b, 2, 17, 0x242070dbu);
  MD5_STEP(MD5_F, b, c, d, a, 3, 22, 0xc1bdceeeu);
  MD5_STEP(MD5_F, a, b, c, d, 4, 7, 0xf57c0fafu);
  MD5_STEP(MD5_F, d, a, b, c, 5, 12, 0x4787c62au);
  MD5_STEP(MD5_F, c, d, a, b, 6, 17, 0xa8304613u);
  MD5_STEP(MD5_F, b, c, d, a, 7, 22, 0xfd469501u);
  MD5_STEP(MD5_F, a, b, c, d, 8, 7, 0x698098d8u);
  MD5_STEP(MD5_F, d, a, b, c, 9, 12, 0x8b44f7afu);
  MD5_STEP(MD5_F, c, d, a, b, 10, 17, 0xffff5bb1u);
  MD5_STEP(MD5_F, b, c, d, a, 11, 22, 0x895cd7beu);
  MD5_STEP(MD5_F, a, b, c, d, 12, 7, 0x6b901122u);
  MD5_STEP(MD5_F, d, a, b, c, 13, 12, 0xfd987193u);
  MD5_STEP(MD5_F, c, d, a, b, 14, 17, 0xa679438eu);
  MD5_STEP(MD5_F, b, c, d, a, 15, 22, 0x49b40821u);

  MD5_STEP(MD5_G, a, b, c, d, 1, 5, 0xf61e2562u);
  MD5_STEP(MD5_G, d, a, b, c, 6, 9, 0xc040b340u);
  MD5_STEP(MD5_G, c, d, a, b, 11, 14, 0x265e5a51u);
  MD5_STEP(MD5_G, b, c, d, a, 0, 20, 0xe9b6c7aau);
  MD5_STEP(MD5_G, a, b, c, d, 5, 5, 0xd62f105du);
  MD5_STEP(MD5_G, d, a, b, c, 10, 9, 0x02441453u);
  MD5_STEP(MD5_G, c, d, a, b, 15, 14, 0xd8a1e681u);
  MD5_STEP(MD5_G, b, c, d, a, 4, 20, 0xe7d3fbc8u);
  MD5_STEP(MD5_G, a, b, c, d, 9, 5, 0x21e1cde6u);
  MD5_STEP(MD5_G, d, a, b, c, 14, 9, 0xc33707d6u);
  MD5_STEP(MD5_G, c, d, a, b, 3, 14, 0xf4d50d87u);
  MD5_STEP(MD5_G, b, c, d, a, 8, 20, 0x455a14edu);
  MD5_STEP(MD5_G, a, b, c, d, 13, 5, 0xa9e3e905u);
  MD5_STEP(MD5_G, d, a, b, c, 2, 9, 0xfcefa3f8u);
  MD5_STEP(MD5_G, c, d, a, b, 7, 14, 0x676f02d9u);
  MD5_STEP(MD5_G, b, c, d, a, 12, 20, 0x8d2a4c8au);

  MD5_STEP(MD5_H, a, b, c, d, 5, 4, 0xfffa3942u);
  MD5_STEP(MD5_H, d, a, b, c, 8, 11, 0x8771f681u);
  MD5_STEP(MD5_H, c, d, a, b, 11, 16, 0x6d9d6122u);
  MD5_STEP(MD5_H, b, c, d, a, 14, 23, 0xfde5380cu);
  MD5_STEP(MD5_H, a, b, c, d, 1, 4, 0xa4beea44u);
  MD5_STEP(MD5_H, d, a, b, c, 4, 11, 0x4bdecfa9u);
  MD5_STEP(MD5_H, c, d, a, b, 7, 16, 0xf6bb4b60u);
  MD5_STEP(MD5_H, b, c, d, a, 10, 23, 0xbebfbc70u);
  MD5_STEP(MD5_H, a, b, c, d, 13, 4, 0x289b7ec6u);
  MD5_STEP(MD5_H, d, a, b, c, 0, 11, 0xeaa127fau);
  MD5_STEP(MD5_H, c, d, a, b, 3, 16, 0xd4ef3085u);
  MD5_STEP(MD5_H, b, c, d, a, 6, 23, 0x04881d05u);
  MD5_STEP(MD5_H, a, b, c, d, 9, 4, 0xd9d4d039u);
  MD5_STEP(MD5_H, d, a, b, c, 12, 11, 0xe6db99e5u);
  MD5_STEP(MD5_H, c, d, a, b, 15, 16, 0x1fa27cf8u);
  MD5_STEP(MD5_H, b, c, d, a, 2, 23, 0xc4ac5665u);

  MD5_STEP(MD5_I, a, b, c, d, 0, 6, 0xf4292244u);
  MD5_STEP(MD5_I, d, a, b, c, 7, 10, 0x432aff97u);
  MD5_STEP(MD5_I, c, d, a, b, 14, 15, 0xab9423a7u);
  MD5_STEP(MD5_I, b, c, d, a, 5, 21, 0xfc93a039u);
  MD5_STEP(MD5_I, a, b, c, d, 12, 6, 0x655b59c3u);
  MD5_STEP(MD5_I, d, a, b, c, 3, 10, 0x8f0ccc92u);
  MD5_STEP(MD5_I, c, d, a, b, 10, 15, 0xffeff47du);
  MD5_STEP(MD5_I, b, c, d, a, 1, 21, 0x85845dd1u);
  MD5_STEP(MD5_I, a, b, c, d, 8, 6, 0x6fa87e4fu);
  MD5_STEP(MD5_I, d, a, b, c, 15, 10, 0xfe2ce6e0u);
  MD5_STEP(MD5_I, c, d, a, b, 6, 15, 0xa3014314u);
  MD5_STEP(MD5_I, b, c, d, a, 13, 21, 0x4e0811a1u);
  MD5_STEP(MD5_I, a, b, c, d, 4, 6, 0xf7537e82u);
  MD5_STEP(MD5_I, d, a, b, c, 11, 10, 0xbd3af235u);
  MD5_STEP(MD5_I, c, d, a, b, 2, 15, 0x2ad7d2bbu);
  MD5_STEP(MD5_I, b, c, d, a, 9, 21, 0xeb86d391u);
  state[0] += a;
  state[1] += b;
  state[2] += c;
  state[3] += d;
}

#undef MD5_STEP
#undef MD5_I
#undef MD5_H
#undef MD5_G
#undef MD5_F

// blocks of a message of `total` bytes: its whole blocks plus one or two padded ones (0x80, zeros, the 8 length bytes)
MD5_HD uint64_t md5_n_blocks(uint64_t total) { return (total >> 6) + ((total & 63u) < 56u ? 1u : 2u); }

// Word j (0..15, a constant where it is called) of the block that starts at byte `pos` (a multiple of 64) of a message
// of `total` bytes, for any block up to the last: message bytes while there are any, then 0x80, zeros, and in the last
// block -- the one the 0x80 and the 8 length bytes end in -- the bit length in words 14 and 15.  `byte_at(i)` gives byte
// i of the message and is asked for i < total only.  (A whole block of data comes out as it is; the kernel takes it this
// way where a wide load would read past the span.)
template <class ByteAt>
MD5_HD uint32_t md5_pad_word(ByteAt byte_at, uint64_t pos, uint64_t total, uint32_t j) {
  const bool last = pos + 64u >= total + 9u;
  if (last && j == 14) return static_cast<uint32_t>(total << 3);
  if (last && j == 15) return static_cast<uint32_t>(total >> 29);  // bits 32..63 of 8 * total
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint64_t i = pos + 4 * j + k;
    uint32_t v = 0;
    if (i < total) v = byte_at(i);
    else if (i == total) v = 0x80u;
    w |= v << (8 * k);
  }
  return w;
}

// The padded blocks behind the whole blocks of a message of `total` bytes, from its n_tail = total % 64 last bytes:
// blocks[0], and blocks[1] when the return value is 2.
MD5_HD uint32_t md5_pad_blocks(const uint8_t* tail, uint32_t n_tail, uint64_t total, uint32_t blocks[2][16]) {
  const uint32_t n = n_tail < 56u ? 1u : 2u;
  const uint64_t first = total - n_tail;
  auto at = [tail, first](uint64_t i) { return static_cast<uint32_t>(tail[i - first]); };
  for (uint32_t b = 0; b < n; ++b)
    for (uint32_t j = 0; j < 16; ++j) blocks[b][j] = md5_pad_word(at, first + 64u * b, total, j);
  return n;
}

// flacenc_hip_md5_spans' table: at most 2^24 spans, each inside [0, n_bytes) -- offset <= n_bytes and
// length <= n_bytes - offset, so that offset + length is never formed and cannot wrap
constexpr uint64_t MAX_SPANS = 1ull << 24;
inline bool spans_inside(const uint64_t* offsets, const uint64_t* lengths, uint64_t n_spans, uint64_t n_bytes) {
  for (uint64_t i = 0; i < n_spans; ++i)
    if (offsets[i] > n_bytes || lengths[i] > n_bytes - offsets[i]) return false;
  return true;
}

MD5_HD void md5_digest(const uint32_t state[4], uint8_t digest[16]) {
  for (uint32_t i = 0; i < 16; ++i) digest[i] = static_cast<uint8_t>(state[i >> 2] >> (8 * (i & 3u)));
}

// the digest of p[0 .. n): reads exactly those bytes
inline void md5_bytes(const uint8_t* p, uint64_t n, uint8_t digest[16]) {
  uint32_t state[4], m[16];
  md5_init(state);
  const uint64_t whole = n >> 6;
  for (uint64_t k = 0; k < whole; ++k) {
    const uint8_t* q = p + 64 * k;
    for (uint32_t j = 0; j < 16; ++j)
      m[j] = static_cast<uint32_t>(q[4 * j]) | static_cast<uint32_t>(q[4 * j + 1]) << 8 |
             static_cast<uint32_t>(q[4 * j + 2]) << 16 | static_cast<uint32_t>(q[4 * j + 3]) << 24;
    md5_block(state, m);
  }
  uint32_t blocks[2][16];
  const uint32_t nb = md5_pad_blocks(n & 63u ? p + 64 * whole : nullptr, static_cast<uint32_t>(n & 63u), n, blocks);
  for (uint32_t b = 0; b < nb; ++b) md5_block(state, blocks[b]);
  md5_digest(state, digest);
}

}  // namespace md5core

#endif  // MD5_CORE_H_
