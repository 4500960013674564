// flac_decode_cpu.cpp -- the host build of flac_decode_core.h: the same parse steps, run one frame per thread.
// Not part of libflacenc_hip.so.  The CPU tests build it with g++ (with and without the address / undefined-behaviour
// sanitizers) to check the core without a GPU, and tools/time_decode.py times it as the CPU baseline:
//   g++ -O2 -std=c++17 -shared -fPIC -pthread flac_decode_cpu.cpp -o libflac_decode_cpu.so
// Arguments and outputs are those of flacenc_hip_decode_frames / _verify_frames / _index_frames (include/flacenc_hip.h).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "flac_decode_core.h"

namespace {

const flacdec::CrcTables kTab = flacdec::make_crc_tables();

// T = int32_t: the narrow decoder; T = int64_t: the wide one (frames of more than flacdec::WIDE_ABOVE_BPS bits)
template <int MAXP, class T>
void decode_row(const uint8_t* p, uint32_t len, uint32_t start, uint32_t bs, uint32_t sbps, T* row) {
  typename flacdec::Decoder<MAXP, sizeof(T) == 8>::type d;
  d.init(p, len, start, bs, sbps);
  for (uint32_t t = 0; t < bs; ++t) row[t] = d.next();
}

template <class T>
void decode_subframe(const uint8_t* p, uint32_t len, uint32_t start, uint32_t bs, uint32_t sbps, T* row) {
  flacdec::BitReader r;
  r.init(p, len, start);
  flacdec::SubInfo si;
  flacdec::parse_subframe_header(r, bs, sbps, si);
  switch (flacdec::order_bucket(si.order)) {
    case 4: decode_row<4>(p, len, start, bs, sbps, row); break;
    case 8: decode_row<8>(p, len, start, bs, sbps, row); break;
    case 16: decode_row<16>(p, len, start, bs, sbps, row); break;
    default: decode_row<32>(p, len, start, bs, sbps, row); break;
  }
}

// one frame: skim, CRC-16, reconstruction; rows of frame f at out + (f*channels + c)*stride (NULL: verify only)
void one_frame(const uint8_t* p, uint32_t len, uint32_t channels, uint32_t bps, uint32_t max_block_size,
               uint32_t max_bps, int32_t* out, const int32_t* expected, size_t stride, uint32_t* block_size,
               uint64_t* number, uint32_t* status, std::vector<int32_t>& tmp, std::vector<int64_t>& wide) {
  flacdec::FrameRec rec;
  uint64_t num = 0;
  flacdec::skim_frame(p, len, channels, bps, max_block_size, max_bps, true, kTab, rec, &num);
  uint32_t st = rec.status;
  if (st == 0 && flacdec::crc16(p, rec.len - 2, kTab) != ((uint32_t(p[rec.len - 2]) << 8) | p[rec.len - 1]))
    st = flacdec::FRAME_CRC;
  const uint32_t bs = st ? 0 : rec.block_size;
  if (st == 0) {
    const uint32_t ch_tag = (rec.info >> 4) & 15u;
    tmp.resize(size_t(channels) * bs);
    if (flacdec::needs_wide(bps)) {  // 64-bit rows, stereo undone in 64 bits, the low 32 bits kept
      wide.resize(size_t(channels) * bs);
      for (uint32_t c = 0; c < channels; ++c)
        decode_subframe(p, len, rec.sub_bit[c], bs, flacdec::subframe_bps(bps, ch_tag, c), wide.data() + size_t(c) * bs);
      if (ch_tag >= 8)
        for (uint32_t t = 0; t < bs; ++t) flacdec::undo_stereo_wide(ch_tag, wide[t], wide[bs + t]);
      for (size_t i = 0; i < wide.size(); ++i) tmp[i] = int32_t(uint32_t(uint64_t(wide[i])));
    } else {
      for (uint32_t c = 0; c < channels; ++c)
        decode_subframe(p, len, rec.sub_bit[c], bs, flacdec::subframe_bps(bps, ch_tag, c), tmp.data() + size_t(c) * bs);
      if (ch_tag >= 8)
        for (uint32_t t = 0; t < bs; ++t) flacdec::undo_stereo(ch_tag, tmp[t], tmp[bs + t]);
    }
    if (expected) {
      for (uint32_t c = 0; c < channels && !(st & flacdec::MISMATCH); ++c)
        if (memcmp(tmp.data() + size_t(c) * bs, expected + c * stride, size_t(bs) * 4) != 0) st |= flacdec::MISMATCH;
    }
  }
  if (out) {
    for (uint32_t c = 0; c < channels; ++c) {
      int32_t* row = out + c * stride;
      if (bs) memcpy(row, tmp.data() + size_t(c) * bs, size_t(bs) * 4);
      memset(row + bs, 0, size_t(max_block_size - bs) * 4);
    }
  }
  if (block_size) *block_size = bs;
  if (number) *number = st ? 0 : num;
  *status = st;
}

}  // namespace

extern "C" {

// decode (out != NULL) or verify (expected != NULL) n_frames frames on `threads` host threads; max_bits_per_sample is
// the depth limit of flacenc_hip_set_max_bits_per_sample, 24 or 32
int fdc_decode_frames_depth(const uint8_t* bytes, const uint64_t* offsets, const uint32_t* lengths, size_t n_frames,
                            uint32_t channels, uint32_t bits_per_sample, uint32_t max_block_size, int32_t* out,
                            const int32_t* expected, size_t stride, uint32_t* block_sizes, uint64_t* numbers,
                            uint32_t* status, int threads, uint32_t max_bits_per_sample) {
  if (max_bits_per_sample != flacdec::MAX_BPS && max_bits_per_sample != flacdec::MAX_BPS_WIDE) return -2;
  if (channels < 1 || channels > flacdec::MAX_CHANNELS || bits_per_sample < 4 || bits_per_sample > max_bits_per_sample ||
      max_block_size < 1 || max_block_size > 65536 || stride < max_block_size)
    return -2;
  std::atomic<size_t> next{0};
  auto work = [&]() {
    std::vector<int32_t> tmp;
    std::vector<int64_t> wide;
    for (size_t f; (f = next.fetch_add(1)) < n_frames;) {
      const size_t row0 = f * channels * stride;
      one_frame(bytes + offsets[f], lengths[f], channels, bits_per_sample, max_block_size, max_bits_per_sample,
                out ? out + row0 : nullptr, expected ? expected + row0 : nullptr, stride,
                block_sizes ? block_sizes + f : nullptr, numbers ? numbers + f : nullptr, status + f, tmp, wide);
    }
  };
  std::vector<std::thread> pool;
  for (int i = 1; i < threads; ++i) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  return 0;
}

int fdc_decode_frames(const uint8_t* bytes, const uint64_t* offsets, const uint32_t* lengths, size_t n_frames,
                      uint32_t channels, uint32_t bits_per_sample, uint32_t max_block_size, int32_t* out,
                      const int32_t* expected, size_t stride, uint32_t* block_sizes, uint64_t* numbers,
                      uint32_t* status, int threads) {
  return fdc_decode_frames_depth(bytes, offsets, lengths, n_frames, channels, bits_per_sample, max_block_size, out,
                                 expected, stride, block_sizes, numbers, status, threads, flacdec::MAX_BPS);
}

// the frames reachable from byte 0 by "the next frame starts where this one ends"; returns 0 when that chain ends
// exactly at n_bytes with at most max_frames frames, 1 otherwise (*n_frames = the frames found up to there)
int fdc_index_frames_depth(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bits_per_sample,
                           size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames,
                           uint32_t max_bits_per_sample) {
  *n_frames = 0;
  uint64_t pos = 0;
  size_t n = 0;
  while (pos < n_bytes) {
    const uint64_t left = n_bytes - pos;
    const uint32_t span = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(left);
    flacdec::FrameRec rec;
    flacdec::skim_frame(bytes + pos, span, channels, bits_per_sample, 65536, max_bits_per_sample, false, kTab, rec,
                        nullptr);
    if (rec.status || flacdec::crc16(bytes + pos, rec.len - 2, kTab) !=
                          ((uint32_t(bytes[pos + rec.len - 2]) << 8) | bytes[pos + rec.len - 1]))
      return 1;
    if (n == max_frames) return 1;
    offsets[n] = pos;
    lengths[n] = rec.len;
    *n_frames = ++n;
    pos += rec.len;
  }
  return 0;
}

int fdc_index_frames(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bits_per_sample,
                     size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames) {
  return fdc_index_frames_depth(bytes, n_bytes, channels, bits_per_sample, max_frames, offsets, lengths, n_frames,
                                flacdec::MAX_BPS);
}

}  // extern "C"

#ifdef FDC_MAIN
// A stand-alone driver for the sanitizer builds (g++ -DFDC_MAIN -fsanitize=address,undefined -static-libasan):
//   fdc in out     in  = u64 n_frames, u32 channels, u32 bits_per_sample, u32 max_block_size, u32 max_bits_per_sample
//                        (0: 24), u64 n_bytes, u64 offsets[n], u32 lengths[n], bytes[n_bytes]
//                  out = u32 status[n], u32 block_sizes[n], i32 samples[n][channels][max_block_size],
//                        then the index of the whole byte buffer: u64 n_found, u32 ok, u64 offsets[n_found]
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0, n_bytes = 0;
  uint32_t hdr[4] = {0, 0, 0, 0};
  if (fread(&n, 8, 1, f) != 1 || fread(hdr, 4, 4, f) != 4 || fread(&n_bytes, 8, 1, f) != 1) return 2;
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  std::vector<uint8_t> bytes(n_bytes);  // exactly n_bytes: any read past the end is an ASan report
  if (fread(off.data(), 8, n, f) != n || fread(len.data(), 4, n, f) != n ||
      fread(bytes.data(), 1, n_bytes, f) != n_bytes)
    return 2;
  fclose(f);
  const uint32_t ch = hdr[0], bps = hdr[1], maxbs = hdr[2], max_bps = hdr[3] ? hdr[3] : flacdec::MAX_BPS;
  std::vector<uint32_t> st(n), bs(n);
  std::vector<int32_t> out(n * ch * maxbs);
  for (uint64_t i = 0; i < n; ++i)
    if (off[i] > n_bytes || len[i] > n_bytes - off[i]) return 3;
  // each frame from a copy of exactly its own bytes, so that a read outside [offset, offset + length) is reported
  std::vector<uint64_t> zero(1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    std::vector<uint8_t> own(bytes.begin() + off[i], bytes.begin() + off[i] + len[i]);
    uint8_t* p = own.empty() ? nullptr : own.data();
    uint8_t dummy = 0;
    if (fdc_decode_frames_depth(p ? p : &dummy, zero.data(), &len[i], 1, ch, bps, maxbs, out.data() + i * ch * maxbs,
                                nullptr, maxbs, &bs[i], nullptr, &st[i], 1, max_bps) != 0)
      return 4;
  }
  std::vector<uint64_t> ioff(n + 64);
  std::vector<uint32_t> ilen(n + 64);
  uint64_t found = 0;
  const uint32_t ok =
      fdc_index_frames_depth(bytes.data(), n_bytes, ch, bps, n + 64, ioff.data(), ilen.data(), &found, max_bps) == 0;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(st.data(), 4, n, o);
  fwrite(bs.data(), 4, n, o);
  fwrite(out.data(), 4, out.size(), o);
  fwrite(&found, 8, 1, o);
  fwrite(&ok, 4, 1, o);
  fwrite(ioff.data(), 8, found, o);
  fclose(o);
  return 0;
}
#endif
