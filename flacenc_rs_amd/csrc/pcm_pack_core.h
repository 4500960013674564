// pcm_pack_core.h -- the index arithmetic of flacenc_hip_pack_le_bytes, shared by the device kernel (pcm_pack.cpp)
// and its host build (pcm_pack_cpu.cpp, compiled by g++ for the CPU tests).
//
// The output of the call is one byte string: frame f's samples start at byte off[f] * channels * B (off the exclusive
// prefix sum of the block sizes, B = bytes_per_sample), sample i of channel c at ((off[f] + i) * channels + c) * B,
// each as the low B bytes of its two's-complement value, little-endian -- the inverse of le_bytes_to_i32s +
// deinterleave (flacenc_hip_fill_le_bytes).  A frame is cut into slices of SLICE samples; a slice is one workgroup's
// span of the output, `ns * channels * B` consecutive bytes that start at any of the four byte alignments:
//
//   split()      the span's head (bytes up to the first aligned dword), its whole dwords and its tail;
//   byte_at()    the value of byte r of the span, for head and tail (byte stores: a neighbouring span owns the rest of
//                that dword, so it is never read, modified and written back);
//   dword_at()   the four bytes r0 .. r0 + 3 of the span as one little-endian word, for the middle (dword stores).
//
// Both take the samples through `load(c, i)`: channel c, sample i of the slice.  They call it for elements of the span
// only -- i < ns -- so nothing beyond a row's block size is ever read.
#ifndef PCM_PACK_CORE_H_
#define PCM_PACK_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define PPK_HD __host__ __device__ inline
#else
#define PPK_HD inline
#endif

namespace pcmpack {

constexpr uint32_t SLICE = 1024;        // samples of one frame that one workgroup moves
constexpr uint32_t MAX_CHANNELS = 8, MAX_BYTES = 4;
constexpr uint32_t MAX_ELEMENTS = SLICE * MAX_CHANNELS;  // samples x channels of a slice

// e / channels for every element index of a slice without a division: (e * magic) >> 16 with magic = ceil(2^16 / C).
// Exact while e * (magic * C - 2^16) < 2^16; magic * C - 2^16 < C <= 8 and e < MAX_ELEMENTS = 2^13, and the product
// stays below 2^29.  (tests/test_pcm_pack_cpu.py checks every e and C.)
PPK_HD uint32_t div_magic(uint32_t channels) { return (65536u + channels - 1u) / channels; }
PPK_HD uint32_t div_channels(uint32_t e, uint32_t magic) { return (e * magic) >> 16; }

// samples of frame `block_size` (already clamped to the stride) that slice `slice` holds: 0 beyond the block
PPK_HD uint32_t slice_samples(uint32_t block_size, uint64_t slice) {
  const uint64_t s0 = slice * SLICE;
  if (s0 >= block_size) return 0;
  const uint64_t left = block_size - s0;
  return left < SLICE ? static_cast<uint32_t>(left) : SLICE;
}

// slices a frame of up to `stride` samples can have
PPK_HD uint64_t slices_per_frame(uint64_t stride) {
  if (stride > 0xFFFFFFFFull) stride = 0xFFFFFFFFull;  // block sizes are 32-bit
  return (stride + SLICE - 1) / SLICE;
}

struct Split {
  uint32_t head;      // bytes in front of the first aligned dword (0..3, never more than the span)
  uint32_t n_dwords;  // whole aligned dwords
  uint32_t tail;      // bytes behind them (0..3)
};

// `low2`: the low two bits of the span's first byte's address
PPK_HD Split split(uint32_t low2, uint32_t len) {
  Split s;
  s.head = (4u - (low2 & 3u)) & 3u;
  if (s.head > len) s.head = len;
  s.n_dwords = (len - s.head) >> 2;
  s.tail = (len - s.head) & 3u;
  return s;
}

template <int B, class Load>
PPK_HD uint32_t byte_at(uint32_t r, uint32_t channels, uint32_t magic, Load load) {
  const uint32_t e = r / B, bb = r - e * B;
  const uint32_t i = div_channels(e, magic), c = e - i * channels;
  return (static_cast<uint32_t>(load(c, i)) >> (8u * bb)) & 0xFFu;
}

// bytes r0 .. r0 + 3, all inside the span: at most four elements, loaded once each, in stream order
template <int B, class Load>
PPK_HD uint32_t dword_at(uint32_t r0, uint32_t channels, uint32_t magic, Load load) {
  const uint32_t e = r0 / B;
  uint32_t bb = r0 - e * B;
  uint32_t i = div_channels(e, magic), c = e - i * channels;
  if (B == 4 && bb == 0) return static_cast<uint32_t>(load(c, i));  // (bb != 0: `out` itself is not dword-aligned)
  uint32_t v = static_cast<uint32_t>(load(c, i)) >> (8u * bb);
  uint32_t w = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < 4; ++j) {
    w |= (v & 0xFFu) << (8u * j);
    v >>= 8;
    if (++bb == static_cast<uint32_t>(B)) {
      bb = 0;
      if (++c == channels) {
        c = 0;
        ++i;
      }
      if (j < 3) v = static_cast<uint32_t>(load(c, i));
    }
  }
  return w;
}

}  // namespace pcmpack

#endif  // PCM_PACK_CORE_H_
