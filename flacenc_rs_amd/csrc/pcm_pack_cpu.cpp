// pcm_pack_cpu.cpp -- the host build of pcm_pack_core.h (g++): a C interface for the CPU tests that walks frames, slices
// and "lanes" exactly as pack_le_bytes_kernel does, and with -DPPK_MAIN a self-checking driver for the sanitizers.
//
//   g++ -O2 -std=c++17 -shared -fPIC pcm_pack_cpu.cpp -o libpcm_pack_cpu.so
//   g++ -O1 -g -std=c++17 -DPPK_MAIN -fsanitize=address,undefined pcm_pack_cpu.cpp -o ppk_san && ./ppk_san
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pcm_pack_core.h"

namespace {

// One slice, as one workgroup moves it.  `addr` is the (pretended) address of out[0]: only its low two bits matter.
// `hits` (NULL to skip) counts the stores per output byte: a byte two spans both wrote would be a race on the device.
template <int B>
void pack_slice(const int32_t* rows, uint64_t stride, uint32_t ns, uint32_t channels, uint8_t* out, uint64_t at,
                uint64_t addr, uint8_t* hits) {
  const uint32_t magic = pcmpack::div_magic(channels);
  auto load = [&](uint32_t c, uint32_t i) { return rows[c * stride + i]; };
  const uint32_t len = ns * channels * B;
  const pcmpack::Split sp = pcmpack::split(static_cast<uint32_t>(addr + at), len);
  auto store = [&](uint64_t r, uint32_t v) {
    out[at + r] = static_cast<uint8_t>(v);
    if (hits) ++hits[at + r];
  };
  for (uint32_t t = 0; t < sp.head; ++t) store(t, pcmpack::byte_at<B>(t, channels, magic, load));
  for (uint32_t k = 0; k < sp.n_dwords; ++k) {
    const uint32_t w = pcmpack::dword_at<B>(sp.head + 4u * k, channels, magic, load);
    for (uint32_t j = 0; j < 4; ++j) store(sp.head + 4u * k + j, w >> (8u * j));
  }
  const uint32_t t0 = sp.head + 4u * sp.n_dwords;
  for (uint32_t t = 0; t < sp.tail; ++t) store(t0 + t, pcmpack::byte_at<B>(t0 + t, channels, magic, load));
}

}  // namespace

extern "C" {

// flacenc_hip_pack_le_bytes on host arrays.  Returns 0, 1 when the output does not fit (nothing written to out), 2 for
// arguments the library rejects.  sample_offsets (n_frames + 1, NULL to skip) and total are always written.
int ppk_pack(const int32_t* frames, uint64_t stride, const uint32_t* block_sizes, uint64_t n_frames, uint32_t channels,
             uint32_t bytes_per_sample, uint8_t* out, uint64_t out_capacity, uint64_t out_addr, uint64_t* sample_offsets,
             uint64_t* total, uint8_t* hits) {
  if (!total || channels < 1 || channels > pcmpack::MAX_CHANNELS || bytes_per_sample < 1 ||
      bytes_per_sample > pcmpack::MAX_BYTES)
    return 2;
  const uint32_t clamp = stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(stride);
  std::vector<uint64_t> off(n_frames + 1, 0);
  for (uint64_t f = 0; f < n_frames; ++f) off[f + 1] = off[f] + (block_sizes[f] < clamp ? block_sizes[f] : clamp);
  if (sample_offsets) memcpy(sample_offsets, off.data(), (n_frames + 1) * 8);
  total[0] = off[n_frames];
  if (off[n_frames] * channels * bytes_per_sample > out_capacity) return 1;
  const uint64_t spf = pcmpack::slices_per_frame(stride);
  for (uint64_t w = 0; w < n_frames * spf; ++w) {
    const uint64_t f = w / spf, sl = w - f * spf;
    const uint32_t bs = block_sizes[f] < clamp ? block_sizes[f] : clamp;
    const uint32_t ns = pcmpack::slice_samples(bs, sl);
    if (ns == 0) continue;
    const uint64_t s0 = sl * pcmpack::SLICE;
    const int32_t* rows = frames + f * channels * stride + s0;
    const uint64_t at = (off[f] + s0) * channels * bytes_per_sample;
    switch (bytes_per_sample) {
      case 1: pack_slice<1>(rows, stride, ns, channels, out, at, out_addr, hits); break;
      case 2: pack_slice<2>(rows, stride, ns, channels, out, at, out_addr, hits); break;
      case 3: pack_slice<3>(rows, stride, ns, channels, out, at, out_addr, hits); break;
      default: pack_slice<4>(rows, stride, ns, channels, out, at, out_addr, hits); break;
    }
  }
  return 0;
}

// the first element index below MAX_ELEMENTS that div_channels gets wrong for `channels`, or -1
int64_t ppk_div_check(uint32_t channels) {
  const uint32_t magic = pcmpack::div_magic(channels);
  for (uint32_t e = 0; e < pcmpack::MAX_ELEMENTS; ++e)
    if (pcmpack::div_channels(e, magic) != e / channels) return e;
  return -1;
}

uint32_t ppk_slice() { return pcmpack::SLICE; }

void ppk_split(uint32_t low2, uint32_t len, uint32_t out[3]) {
  const pcmpack::Split s = pcmpack::split(low2, len);
  out[0] = s.head;
  out[1] = s.n_dwords;
  out[2] = s.tail;
}

}  // extern "C"

#ifdef PPK_MAIN
#include <stdio.h>

// Every width, channel count and alignment over block-size lists with empty, tiny, slice-sized and ragged frames, rows
// and outputs in exact-size heap blocks (a read or a store one element out is an ASan report), against the plain
// statement of the layout; sentinels behind every row's block size must not reach the output.
int main() {
  const uint32_t lists[][7] = {{0, 1, 2, 3, 5, 0, 16}, {63, 64, 255, 256, 257, 1, 0}, {1024, 1025, 3, 2047, 0, 2048, 7},
                               {4096, 1, 1, 1, 4097, 0, 2}};
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  int cases = 0;
  for (const auto& list : lists)
    for (uint32_t channels = 1; channels <= 8; ++channels)
      for (uint32_t B = 1; B <= 4; ++B)
        for (uint32_t pad = 0; pad < 2; ++pad) {
          const uint64_t n_frames = 7;
          uint32_t biggest = 0;
          for (uint32_t b : list) biggest = b > biggest ? b : biggest;
          const uint64_t stride = biggest + pad * 5;
          std::vector<int32_t> rows(n_frames * channels * stride);
          std::vector<uint32_t> bs(list, list + 7);
          if (pad) bs[3] = static_cast<uint32_t>(stride) + 1000u;  // garbage above the stride counts as the stride
          for (uint64_t f = 0; f < n_frames; ++f)
            for (uint32_t c = 0; c < channels; ++c)
              for (uint64_t i = 0; i < stride; ++i)
                rows[(f * channels + c) * stride + i] = static_cast<int32_t>(next());
          uint64_t total = 0;
          for (uint32_t b : bs) total += b < stride ? b : stride;
          const uint64_t nbytes = total * channels * B;
          std::vector<uint8_t> want(nbytes), got(nbytes, 0xEE), hits(nbytes, 0);
          uint64_t at = 0;
          for (uint64_t f = 0; f < n_frames; ++f) {
            const uint64_t n = bs[f] < stride ? bs[f] : stride;
            for (uint64_t i = 0; i < n; ++i)
              for (uint32_t c = 0; c < channels; ++c) {
                const uint32_t v = static_cast<uint32_t>(rows[(f * channels + c) * stride + i]);
                for (uint32_t b = 0; b < B; ++b) want[at++] = static_cast<uint8_t>(v >> (8 * b));
              }
          }
          for (uint64_t addr = 0; addr < 4; ++addr) {
            std::vector<uint64_t> offs(n_frames + 1);
            uint64_t t = 0;
            std::fill(hits.begin(), hits.end(), 0);
            const int rc = ppk_pack(rows.data(), stride, bs.data(), n_frames, channels, B, got.data(), nbytes, addr,
                                    offs.data(), &t, hits.data());
            if (rc != 0 || t != total || offs[n_frames] != total || got != want) {
              printf("FAIL: channels %u bytes %u pad %u addr %llu rc %d\n", channels, B, pad, (unsigned long long)addr, rc);
              return 1;
            }
            for (uint8_t hcount : hits)
              if (hcount != 1) {
                printf("FAIL: a byte stored %u times (channels %u bytes %u)\n", hcount, channels, B);
                return 1;
              }
            ++cases;
          }
          // one byte short: nothing is written, the total still is
          if (nbytes) {
            std::vector<uint8_t> small(nbytes - 1, 0xEE);
            uint64_t t = 0;
            if (ppk_pack(rows.data(), stride, bs.data(), n_frames, channels, B, small.data(), nbytes - 1, 0, nullptr, &t,
                         nullptr) != 1 || t != total) {
              printf("FAIL: short capacity\n");
              return 1;
            }
            for (uint8_t v : small)
              if (v != 0xEE) {
                printf("FAIL: short capacity wrote\n");
                return 1;
              }
          }
        }
  for (uint32_t c = 1; c <= 8; ++c)
    if (ppk_div_check(c) != -1) {
      printf("FAIL: div_channels(%u)\n", c);
      return 1;
    }
  printf("pcm_pack_cpu self-check OK: %d cases\n", cases);
  return 0;
}
#endif
