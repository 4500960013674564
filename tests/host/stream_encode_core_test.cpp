// stream_encode_core_test.cpp -- csrc/stream_encode_core.h as a stand-alone program for the address and
// undefined-behaviour sanitizers (tests/test_encode_streams_cpu.py builds and runs it; the files it reads and writes are
// that test's):
//   renumber <vectors>   every record is a frame the oracle wrote with number 0 and, for a list of numbers, the frame the
//                        oracle wrote with that number: renumber_frame must give it byte for byte (header, CRC-8, the
//                        CRC-16 by combination, the length), renumbered_length and renumbered_header_bytes must agree,
//                        and the device's form of x^(8|B|) -- the product of XPOW8 over |B|'s set bits -- must give the
//                        same CRC-16
//   plan <tables> <out>  build_plan on every table of the file, written out field by field for the test's brute-force
//                        statement; the invariants that need no second opinion are checked here
//   checks               check_streams and count_frames on the rejections the call documents
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_encode_core.h"

typedef flacenc_hip_pcm_stream_desc Desc;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      if (++failures > 20) std::exit(1);                              \
    }                                                                 \
  } while (0)

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::printf("cannot open %s\n", path);
    std::exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

struct Reader {
  const std::vector<uint8_t>& v;
  size_t at = 0;
  uint64_t u64() {
    uint64_t x = 0;
    CHECK(at + 8 <= v.size());
    std::memcpy(&x, v.data() + at, 8);
    at += 8;
    return x;
  }
  uint32_t u32() {
    uint32_t x = 0;
    CHECK(at + 4 <= v.size());
    std::memcpy(&x, v.data() + at, 4);
    at += 4;
    return x;
  }
  std::vector<uint8_t> bytes(size_t n) {
    CHECK(at + n <= v.size());
    std::vector<uint8_t> b(v.begin() + at, v.begin() + at + n);
    at += n;
    return b;
  }
};

// vectors: u32 records; per record u32 len0, frame0, u32 k, then k x (u32 number, u32 len, frame)
static int run_renumber(const char* path) {
  const std::vector<uint8_t> file = read_file(path);
  Reader r{file};
  const vbs::XPow8 xp = vbs::make_xpow8();
  const uint32_t records = r.u32();
  uint32_t checked = 0;
  for (uint32_t i = 0; i < records; ++i) {
    const uint32_t len0 = r.u32();
    const std::vector<uint8_t> f0 = r.bytes(len0);
    const uint32_t k = r.u32();
    for (uint32_t j = 0; j < k; ++j) {
      const uint32_t number = r.u32(), len = r.u32();
      const std::vector<uint8_t> want = r.bytes(len);
      std::vector<uint8_t> got(len0 + 5, 0xEE);  // exactly the room the function asks for
      const uint32_t n = streamenc::renumber_frame(f0.data(), len0, number, got.data());
      CHECK(n == len);
      CHECK(n == streamenc::renumbered_length(len0, number));
      CHECK(n <= got.size() && std::memcmp(got.data(), want.data(), n < len ? n : len) == 0);
      for (size_t b = n; b < got.size(); ++b) CHECK(got[b] == 0xEE);
      const uint32_t hf = vbs::header_bytes(f0.data());
      const uint32_t hv = streamenc::renumbered_header_bytes(f0.data(), number);
      uint8_t hd[16];
      CHECK(streamenc::write_renumbered_header(f0.data(), number, hd) == hv && hv - hf == len - len0);
      CHECK(hv == vbs::header_bytes(want.data()) && std::memcmp(hd, want.data(), hv) == 0);
      // the device's form of x^(8|B|)
      const uint32_t body = len0 - 2u - hf;
      uint32_t p = 1;
      for (int bit = 0; bit < 32; ++bit)
        if ((body >> bit) & 1u) p = flacdec::crc16_mulmod(p, xp.v[bit]);
      const uint32_t crc_old = (static_cast<uint32_t>(f0[len0 - 2]) << 8) | f0[len0 - 1];
      const uint32_t crc = vbs::crc16_combine(crc_old, vbs::crc16_bytes(f0.data(), hf), vbs::crc16_bytes(hd, hv), p);
      CHECK(crc == ((static_cast<uint32_t>(want[len - 2]) << 8) | want[len - 1]));
      CHECK(crc == vbs::crc16_bytes(want.data(), len - 2));
      ++checked;
    }
  }
  CHECK(r.at == file.size());
  // a frame too short to be one, a first byte that starts no coded number
  uint8_t junk[8] = {0xFF, 0xF8, 0x19, 0x08, 0x80, 0, 0, 0}, out[16];
  CHECK(streamenc::renumber_frame(junk, 8, 3, out) == 0 && streamenc::write_renumbered_header(junk, 3, out) == 0);
  junk[4] = 0;
  CHECK(streamenc::renumber_frame(junk, 7, 3, out) == 0);
  if (failures) return 1;
  std::printf("renumber OK %u\n", checked);
  return 0;
}

static size_t fake_bound(uint32_t channels, uint32_t n, uint32_t bits) { return 15 + (channels * (8 + n * bits) + 7) / 8 + 2; }

// tables: u32 tables; per table u32 block_size, u32 chunk, u32 n, n x Desc (48 bytes)
// out: per table u64 frames, then per launch position (u64 pcm_offset, u32 valid, u32 stream_pos), per stream position
// (u64 pack_offset, u32 launch_pos, u32 stream, u32 index), n + 1 x u32 stream_first, u32 classes, per class 9 words
// (u64 each), u32 runs, per run 4 x u32, u32 full_runs, u32 tail_runs, u64 pack_bytes, u64 max_class_rows
static int run_plan(const char* in_path, const char* out_path) {
  const std::vector<uint8_t> file = read_file(in_path);
  Reader r{file};
  FILE* o = std::fopen(out_path, "wb");
  if (!o) return 2;
  auto w32 = [&](uint32_t x) { std::fwrite(&x, 4, 1, o); };
  auto w64 = [&](uint64_t x) { std::fwrite(&x, 8, 1, o); };
  const uint32_t tables = r.u32();
  for (uint32_t t = 0; t < tables; ++t) {
    const uint32_t block = r.u32(), chunk = r.u32(), n = r.u32();
    std::vector<Desc> d(n);
    for (uint32_t s = 0; s < n; ++s) {
      const std::vector<uint8_t> b = r.bytes(sizeof(Desc));
      std::memcpy(&d[s], b.data(), sizeof(Desc));
    }
    const uint64_t frames = streamenc::count_frames(d.data(), n, block);
    CHECK(streamenc::check_streams(d.data(), n, ~0ull >> 1, ~0ull >> 1, block) == FLACENC_HIP_OK);
    const streamenc::Plan pl = streamenc::build_plan(d.data(), n, block, [&](const streamenc::Class&) { return chunk; }, fake_bound);
    CHECK(pl.launch.size() == frames && pl.stream.size() == frames && pl.stream_first.size() == n + 1u);
    // the two orders are permutations of each other
    for (uint32_t p = 0; p < frames; ++p) CHECK(pl.launch[p].stream_pos < frames && pl.stream[pl.launch[p].stream_pos].launch_pos == p);
    // runs tile the launch order, stay inside one class, hold frames of one length and at most `chunk` of them
    uint32_t at = 0;
    for (const streamenc::Run& run : pl.runs) {
      CHECK(run.first == at && run.frames >= 1 && run.frames <= chunk);
      const streamenc::Class& k = pl.classes[run.cls];
      CHECK(run.first >= k.first && run.first + run.frames <= k.first + k.full + k.tails);
      for (uint32_t p = run.first; p < run.first + run.frames; ++p) CHECK(pl.launch[p].valid == run.block);
      at += run.frames;
    }
    CHECK(at == frames && pl.runs.size() == pl.full_runs + pl.tail_runs);
    // pack slots: 16-byte aligned, disjoint, inside pack_bytes
    for (uint32_t q = 0; q < frames; ++q) {
      const streamenc::StreamFrame& f = pl.stream[q];
      const streamenc::Class* k = nullptr;
      for (const streamenc::Class& c : pl.classes)
        if (f.launch_pos >= c.first && f.launch_pos < c.first + c.full + c.tails) k = &c;
      CHECK(k && f.pack_offset % 16 == 0 && f.pack_offset == k->pack_base + (uint64_t)(f.launch_pos - k->first) * k->pack_stride);
      CHECK(f.pack_offset + k->pack_stride <= pl.pack_bytes && f.pack_room == k->pack_stride);
      CHECK(k->pack_stride >= fake_bound(k->channels, block, k->bits_per_sample));
    }
    w64(frames);
    for (const streamenc::LaunchFrame& f : pl.launch) {
      w64(f.pcm_offset);
      w32(f.valid);
      w32(f.stream_pos);
    }
    for (const streamenc::StreamFrame& f : pl.stream) {
      w64(f.pack_offset);
      w32(f.launch_pos);
      w32(f.stream);
      w32(f.index);
    }
    for (uint32_t v : pl.stream_first) w32(v);
    w32(static_cast<uint32_t>(pl.classes.size()));
    for (const streamenc::Class& k : pl.classes)
      for (uint64_t v : {(uint64_t)k.channels, (uint64_t)k.bits_per_sample, (uint64_t)k.bytes_per_sample, (uint64_t)k.sample_rate,
                         (uint64_t)k.first, (uint64_t)k.full, (uint64_t)k.tails, k.pack_base, k.pack_stride})
        w64(v);
    w32(static_cast<uint32_t>(pl.runs.size()));
    for (const streamenc::Run& run : pl.runs) {
      w32(run.first);
      w32(run.frames);
      w32(run.block);
      w32(run.cls);
    }
    w32(pl.full_runs);
    w32(pl.tail_runs);
    w64(pl.pack_bytes);
    w64(pl.max_class_rows);
  }
  CHECK(r.at == file.size());
  std::fclose(o);
  if (failures) return 1;
  std::printf("plan OK %u\n", tables);
  return 0;
}

static Desc desc(uint64_t off, uint64_t samples, uint64_t out_off, uint64_t cap, uint32_t ch = 2, uint32_t bits = 16,
                 uint32_t bytes = 2) {
  Desc d{};
  d.offset = off;
  d.total_samples = samples;
  d.out_offset = out_off;
  d.out_capacity = cap;
  d.channels = ch;
  d.bits_per_sample = bits;
  d.bytes_per_sample = bytes;
  d.sample_rate = 44100;
  return d;
}

static int run_checks() {
  const int BAD = FLACENC_HIP_ERR_BAD_ARGUMENT;
  Desc ok = desc(3, 100, 8, 40);
  CHECK(streamenc::check_streams(&ok, 1, 403, 48, 64) == FLACENC_HIP_OK);
  CHECK(streamenc::check_streams(&ok, 1, 402, 48, 64) == BAD);   // the span ends one byte past pcm_bytes
  CHECK(streamenc::check_streams(&ok, 1, 403, 47, 64) == BAD);   // the slot ends one byte past out_bytes
  CHECK(streamenc::check_streams(&ok, 1, 403, 48, 63) == BAD && streamenc::check_streams(&ok, 1, 403, 48, 32768) == BAD);
  CHECK(streamenc::check_streams(&ok, 1, 403, 48, 32767) == FLACENC_HIP_OK);
  CHECK(streamenc::check_streams(nullptr, 0, 0, 0, 4096) == FLACENC_HIP_OK);
  Desc empty = desc(0, 0, 0, 0);
  CHECK(streamenc::check_streams(&empty, 1, 0, 0, 4096) == FLACENC_HIP_OK && streamenc::count_frames(&empty, 1, 4096) == 0);
  for (uint32_t ch : {0u, 9u}) {
    Desc d = desc(0, 1, 0, 0, ch);
    CHECK(streamenc::check_streams(&d, 1, 1000, 0, 4096) == BAD);
  }
  for (uint32_t bytes : {0u, 5u}) {
    Desc d = desc(0, 1, 0, 0, 2, 16, bytes);
    CHECK(streamenc::check_streams(&d, 1, 1000, 0, 4096) == BAD);
  }
  for (uint32_t bits : {7u, 25u}) {
    Desc d = desc(0, 1, 0, 0, 2, bits);
    CHECK(streamenc::check_streams(&d, 1, 1000, 0, 4096) == BAD);
  }
  // overflow: offset + bytes wraps, total_samples * per wraps
  Desc wrap = desc(~0ull - 3, 2, 0, 0);
  CHECK(streamenc::check_streams(&wrap, 1, ~0ull, 0, 4096) == BAD);
  Desc huge = desc(0, ~0ull / 2, 0, 0);
  CHECK(streamenc::check_streams(&huge, 1, ~0ull, 0, 4096) == BAD);
  Desc slot = desc(0, 0, ~0ull - 1, 4);
  CHECK(streamenc::check_streams(&slot, 1, 0, ~0ull, 4096) == BAD);
  // 2^31 frames: one too many; 2^31 - 1 passes (mono, one byte per sample, block 64)
  Desc many = desc(0, (1ull << 31) * 64 - 64 + 1, 0, 0, 1, 8, 1);
  CHECK(streamenc::count_frames(&many, 1, 64) == 1ull << 31);
  CHECK(streamenc::check_streams(&many, 1, 1ull << 40, 0, 64) == BAD);
  many.total_samples -= 1;
  CHECK(streamenc::count_frames(&many, 1, 64) == (1ull << 31) - 1);
  CHECK(streamenc::check_streams(&many, 1, 1ull << 40, 0, 64) == FLACENC_HIP_OK);
  // frame counts: 0, exactly k blocks, tails of 1, 63, 64
  const uint64_t samples[] = {0, 4096, 8192, 4097, 4096 + 63, 4096 + 64, 1, 63, 64};
  const uint64_t frames[] = {0, 1, 2, 2, 2, 2, 1, 1, 1};
  std::vector<Desc> t;
  uint64_t sum = 0;
  for (int i = 0; i < 9; ++i) {
    t.push_back(desc(0, samples[i], 0, 0));
    CHECK(streamenc::frames_of(samples[i], 4096) == frames[i]);
    sum += frames[i];
  }
  CHECK(streamenc::count_frames(t.data(), t.size(), 4096) == sum);
  CHECK(streamenc::count_frames(t.data(), t.size(), 0) == 0 && streamenc::count_frames(nullptr, 3, 64) == 0);
  // coded number seams
  const uint32_t numbers[] = {0, 127, 128, 2047, 2048, 65535, 65536, (1u << 21) - 1, 1u << 21, (1u << 26) - 1, 1u << 26, 0x7FFFFFFFu};
  const uint32_t coded[] = {1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};
  for (int i = 0; i < 12; ++i) CHECK(streamenc::renumbered_length(100, numbers[i]) == 99 + coded[i]);
  if (failures) return 1;
  std::printf("checks OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "renumber")) return run_renumber(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "plan")) return run_plan(argv[2], argv[3]);
  if (argc == 2 && !std::strcmp(argv[1], "checks")) return run_checks();
  std::printf("usage: renumber <vectors> | plan <tables> <out> | checks\n");
  return 2;
}
