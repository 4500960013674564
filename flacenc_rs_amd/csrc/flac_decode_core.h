// flac_decode_core.h -- the FLAC frame parser shared by the device decoder (flac_decode.cpp) and its host build
// (flac_decode_cpu.cpp, compiled by g++ for the CPU tests and the CPU baseline).
//
// RFC 9639 frames: both sync codes, every block-size and sample-rate code, channel codes 0..10, the coded number up
// to 7 bytes, CRC-8; Constant, Verbatim, Fixed 0..4 and LPC 1..32 subframes with wasted bits; both Rice methods with
// escaped partitions.  Everything here is bounded by the frame: the bit reader never touches a byte outside
// [p, p + len) and raises `over` instead, and every loop runs at most block-size times (or the frame's bit count).
//
// The parse is split so that the device can spread it: skim_frame walks a frame's codes without reconstructing and
// records where each subframe starts; SubDecoder<MAXP> then reconstructs one subframe from its start bit.  The host
// build runs the same two steps one after the other, so both builds give the same status for the same bytes.
#ifndef FLAC_DECODE_CORE_H_
#define FLAC_DECODE_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FD_HD __host__ __device__ inline
#else
#define FD_HD inline
#endif
#if defined(__clang__)
#define FD_UNROLL _Pragma("unroll")
#else
#define FD_UNROLL _Pragma("GCC unroll 32")
#endif

namespace flacdec {

// status bits (FLACENC_HIP_DECODE_* in include/flacenc_hip.h)
constexpr uint32_t BAD_HEADER = 1u, HEADER_CRC = 2u, FRAME_CRC = 4u, PARSE = 8u, LENGTH = 16u, STREAM_MISMATCH = 32u,
                   UNSUPPORTED = 64u, MISMATCH = 128u;
constexpr uint32_t MAX_CHANNELS = 8;
// The depth limit is the caller's (flacenc_hip_set_max_bits_per_sample): MAX_BPS is the default and what callers without
// a handle pass, MAX_BPS_WIDE the most the format allows.  A frame deeper than WIDE_ABOVE_BPS is reconstructed by the
// wide decoder (WideSubDecoder below), every other frame by SubDecoder.
constexpr uint32_t MAX_BPS = 24, MAX_BPS_WIDE = 32, WIDE_ABOVE_BPS = 24;

// ---- CRCs (RFC 9639 section 9.1.8: CRC-8 poly 0x07, section 9.3: CRC-16 poly 0x8005; MSB first, init 0) ----
struct CrcTables {
  uint8_t t8[256];
  uint16_t t16[256];
  uint16_t klo[256], khi[256];  // b * x^2048 mod P and (b << 8) * x^2048 mod P: advance a CRC-16 by 256 zero bytes
  uint16_t xp[64];              // x^(8 * (252 - 4 i)) mod P: the tail shift of lane i in crc16_kernel
};

constexpr uint32_t crc16_mulmod(uint32_t a, uint32_t b) {
  uint32_t prod = 0;
  for (int j = 0; j < 16; ++j)
    if ((b >> j) & 1u) prod ^= a << j;
  for (int k = 31; k >= 16; --k)
    if ((prod >> k) & 1u) prod ^= 0x18005u << (k - 16);
  return prod & 0xFFFFu;
}

constexpr uint32_t crc16_xpow(uint32_t n) {  // x^n mod P
  uint32_t r = 1, base = 2;
  while (n) {
    if (n & 1u) r = crc16_mulmod(r, base);
    base = crc16_mulmod(base, base);
    n >>= 1;
  }
  return r;
}

constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c8 = i, c16 = i << 8;
    for (int k = 0; k < 8; ++k) {
      c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
      c16 = (c16 & 0x8000u) ? ((c16 << 1) ^ 0x8005u) & 0xFFFFu : (c16 << 1) & 0xFFFFu;
    }
    t.t8[i] = static_cast<uint8_t>(c8);
    t.t16[i] = static_cast<uint16_t>(c16);
  }
  const uint32_t k = crc16_xpow(2048);
  for (uint32_t b = 0; b < 256; ++b) {
    t.klo[b] = static_cast<uint16_t>(crc16_mulmod(b, k));
    t.khi[b] = static_cast<uint16_t>(crc16_mulmod(b << 8, k));
  }
  for (uint32_t i = 0; i < 64; ++i) t.xp[i] = static_cast<uint16_t>(crc16_xpow(8 * (252 - 4 * i)));
  return t;
}

// ---- bit reader: MSB first, clamped to [p, p + len) ----
struct BitReader {
  const uint8_t* p;
  uint32_t len;   // bytes
  uint32_t next;  // next byte to enter the cache
  int cnt;        // valid bits in cache (left-aligned)
  bool over;      // a read went past the end of the frame
  uint64_t cache;

  // whole aligned words where they fit, single bytes to reach alignment and at the end of the frame
  FD_HD void refill() {
    while (cnt <= 56 && next < len) {
      if (cnt <= 32 && next + 4 <= len && (reinterpret_cast<uintptr_t>(p + next) & 3u) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + next);
        const uint32_t be = (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24);
        cache |= static_cast<uint64_t>(be) << (32 - cnt);
        cnt += 32;
        next += 4;
      } else {
        cache |= static_cast<uint64_t>(p[next++]) << (56 - cnt);
        cnt += 8;
      }
    }
  }
  FD_HD void init(const uint8_t* base, uint32_t n, uint64_t bit) {
    p = base;
    len = n;
    over = false;
    cache = 0;
    cnt = 0;
    if ((bit >> 3) >= n) {
      next = n;
      over = bit > static_cast<uint64_t>(n) * 8;
      return;
    }
    next = static_cast<uint32_t>(bit >> 3);
    refill();
    skip(static_cast<uint32_t>(bit & 7u));
  }
  FD_HD uint64_t pos() const { return static_cast<uint64_t>(next) * 8 - static_cast<uint64_t>(cnt); }
  FD_HD uint32_t u(uint32_t n) {  // n <= 32
    if (n == 0) return 0;
    if (cnt < static_cast<int>(n)) refill();
    if (cnt < static_cast<int>(n)) {
      over = true;
      cache = 0;
      cnt = 0;
      return 0;
    }
    const uint32_t v = static_cast<uint32_t>(cache >> (64 - n));
    cache = n == 64 ? 0 : cache << n;
    cnt -= static_cast<int>(n);
    return v;
  }
  FD_HD int32_t s(uint32_t n) {  // two's complement, n <= 32
    const uint32_t v = u(n);
    if (n == 0 || n == 32) return static_cast<int32_t>(v);
    return static_cast<int32_t>(v << (32 - n)) >> (32 - n);
  }
  FD_HD int64_t s64(uint32_t n) {  // two's complement, n <= 33: the samples of a 33-bit side subframe
    if (n <= 32) return s(n);
    const uint64_t hi = u(n - 32);  // two reads, so that u() keeps its 32-bit contract
    const uint64_t v = (hi << 32) | u(32);
    return static_cast<int64_t>(v << (64 - n)) >> (64 - n);
  }
  FD_HD void skip(uint32_t n) {
    while (n > 32) {
      u(32);
      n -= 32;
    }
    u(n);
  }
  FD_HD void skip_bits(uint64_t n) {  // bounded by the frame: a long skip past the end only sets `over`
    const uint64_t left = static_cast<uint64_t>(len) * 8 - pos();
    if (n > left) {
      over = true;
      next = len;
      cache = 0;
      cnt = 0;
      return;
    }
    const uint64_t target = pos() + n;
    if (n > 64) {
      next = static_cast<uint32_t>(target >> 3);
      cache = 0;
      cnt = 0;
      refill();
      skip(static_cast<uint32_t>(target & 7u));
    } else {
      skip(static_cast<uint32_t>(n));
    }
  }
  // number of 0 bits before the next 1 (consumed); `over` when the frame ends first
  FD_HD uint32_t unary() {
    uint32_t q = 0;
    for (;;) {
      if (cnt < 64) refill();
      if (cnt == 0) {
        over = true;
        return q;
      }
      if (cache == 0) {
        q += static_cast<uint32_t>(cnt);
        cnt = 0;
        continue;
      }
      const int z = __builtin_clzll(cache);
      q += static_cast<uint32_t>(z);
      cache = z == 63 ? 0 : cache << (z + 1);  // z < cnt <= 64
      cnt -= z + 1;
      return q;
    }
  }
};

// ---- frame header ----
struct Header {
  uint32_t block_size, channels, ch_tag, bps, header_bytes, variable;
  uint64_t number;
};

// `len` is what the frame may occupy; status 0 or BAD_HEADER / HEADER_CRC / STREAM_MISMATCH / UNSUPPORTED.  max_bps is
// the depth limit: a header that says more bits per sample is UNSUPPORTED.
FD_HD uint32_t parse_header(const uint8_t* p, uint32_t len, uint32_t channels, uint32_t bits_per_sample,
                            uint32_t max_block_size, uint32_t max_bps, const CrcTables& tab, Header& h) {
  BitReader r;
  r.init(p, len, 0);
  if (r.u(15) != 0x7FFCu) return BAD_HEADER;  // 14-bit sync + the reserved bit
  h.variable = r.u(1);
  const uint32_t bs_code = r.u(4), sr_code = r.u(4), ch_code = r.u(4), ss_code = r.u(3);
  if (r.u(1) != 0) return BAD_HEADER;
  if (bs_code == 0 || sr_code == 15 || ch_code > 10 || ss_code == 3) return BAD_HEADER;
  const uint32_t first = r.u(8);
  uint32_t ones = 0;
  while (ones < 8 && ((first >> (7 - ones)) & 1u)) ++ones;
  if (ones == 1 || ones == 8) return BAD_HEADER;
  uint64_t number = ones == 0 ? first : (first & ((1u << (7 - ones)) - 1u));
  for (uint32_t i = 1; i < ones; ++i) {
    const uint32_t b = r.u(8);
    if ((b >> 6) != 2u) return BAD_HEADER;
    number = (number << 6) | (b & 0x3Fu);
  }
  h.number = number;
  uint32_t bs;
  if (bs_code == 1) bs = 192;
  else if (bs_code <= 5) bs = 576u << (bs_code - 2);
  else if (bs_code == 6) bs = r.u(8) + 1;
  else if (bs_code == 7) bs = r.u(16) + 1;
  else bs = 256u << (bs_code - 8);
  if (sr_code == 12) r.u(8);
  else if (sr_code == 13 || sr_code == 14) r.u(16);
  if (r.over) return BAD_HEADER;
  const uint32_t hlen = static_cast<uint32_t>(r.pos() >> 3);
  const uint32_t crc = r.u(8);
  if (r.over) return BAD_HEADER;
  uint32_t c8 = 0;
  for (uint32_t i = 0; i < hlen; ++i) c8 = tab.t8[c8 ^ p[i]];
  if (c8 != crc) return HEADER_CRC;
  h.header_bytes = hlen + 1;
  h.block_size = bs;
  h.ch_tag = ch_code;
  h.channels = ch_code < 8 ? ch_code + 1 : 2;
  h.bps = ss_code == 0 ? bits_per_sample
          : ss_code == 1 ? 8u
          : ss_code == 2 ? 12u
          : ss_code == 4 ? 16u
          : ss_code == 5 ? 20u
          : ss_code == 6 ? 24u
                         : 32u;
  uint32_t st = 0;
  if (h.channels != channels || h.bps != bits_per_sample) st |= STREAM_MISMATCH;
  if (h.bps > max_bps || bs > max_block_size) st |= UNSUPPORTED;
  return st;
}

// ---- subframes ----
enum : uint32_t { KIND_CONSTANT = 0, KIND_VERBATIM = 1, KIND_FIXED = 2, KIND_LPC = 3 };

struct SubInfo {
  uint32_t kind, order, wasted, ebps;
};

// bits per sample of channel c under channel code ch_tag (the side channel carries one more)
FD_HD uint32_t subframe_bps(uint32_t bps, uint32_t ch_tag, uint32_t c) {
  const bool side = (ch_tag == 8 && c == 1) || (ch_tag == 9 && c == 0) || (ch_tag == 10 && c == 1);
  return bps + (side ? 1u : 0u);
}

FD_HD uint32_t parse_subframe_header(BitReader& r, uint32_t bs, uint32_t sbps, SubInfo& si) {
  if (r.u(1) != 0) return PARSE;
  const uint32_t type = r.u(6);
  si.wasted = r.u(1) ? r.unary() + 1 : 0;
  if (r.over || si.wasted >= sbps) return PARSE;
  si.ebps = sbps - si.wasted;
  if (type == 0) {
    si.kind = KIND_CONSTANT;
    si.order = 0;
  } else if (type == 1) {
    si.kind = KIND_VERBATIM;
    si.order = 0;
  } else if (type >= 8 && type <= 12) {
    si.kind = KIND_FIXED;
    si.order = type - 8;
  } else if (type >= 32) {
    si.kind = KIND_LPC;
    si.order = type - 31;
  } else {
    return PARSE;
  }
  if (si.order > bs) return PARSE;
  return 0;
}

// the residual's partition header: method, order; 0 or PARSE
struct ResidualState {
  uint32_t pbits, esc, nparts, part_size, part, left, param, escaped;
};

FD_HD uint32_t residual_begin(BitReader& r, uint32_t bs, uint32_t order, ResidualState& rs) {
  const uint32_t method = r.u(2);
  if (method > 1) return PARSE;
  rs.pbits = method ? 5 : 4;
  rs.esc = method ? 31 : 15;
  const uint32_t po = r.u(4);
  rs.nparts = 1u << po;
  rs.part_size = bs >> po;
  if ((rs.part_size << po) != bs || rs.part_size < order) return PARSE;
  rs.part = 0;
  rs.left = 0;
  rs.param = 0;
  rs.escaped = 0;
  return r.over ? PARSE : 0;
}

// reads the next partition's header; 0 or PARSE
FD_HD uint32_t residual_open(BitReader& r, uint32_t order, ResidualState& rs) {
  if (rs.part >= rs.nparts) return PARSE;
  const uint32_t p = r.u(rs.pbits);
  if (p == rs.esc) {
    rs.escaped = 1;
    rs.param = r.u(5);
  } else {
    rs.escaped = 0;
    rs.param = p;
  }
  rs.left = rs.part == 0 ? rs.part_size - order : rs.part_size;
  ++rs.part;
  return r.over ? PARSE : 0;
}

// opens partitions until one has samples left (only partition 0 can hold none); 0 or PARSE
FD_HD uint32_t residual_partition(BitReader& r, uint32_t order, ResidualState& rs) {
  while (rs.left == 0)
    if (residual_open(r, order, rs)) return PARSE;
  return 0;
}

// one residual of the open partition (caller has called residual_partition); sets *bad on an out-of-range code
FD_HD int32_t residual_next(BitReader& r, ResidualState& rs, uint32_t* bad) {
  --rs.left;
  if (rs.escaped) return r.s(rs.param);
  const uint32_t q = r.unary();
  const uint64_t v = (static_cast<uint64_t>(q) << rs.param) | r.u(rs.param);
  if ((v >> 32) != 0 || q > 0xFFFFFFFEu) *bad = PARSE;
  const uint32_t u = static_cast<uint32_t>(v);
  return static_cast<int32_t>((u >> 1) ^ (0u - (u & 1u)));
}

// walks one subframe without reconstructing; 0 or PARSE
FD_HD uint32_t skim_subframe(BitReader& r, uint32_t bs, uint32_t sbps) {
  SubInfo si;
  if (parse_subframe_header(r, bs, sbps, si)) return PARSE;
  if (si.kind == KIND_CONSTANT) {
    r.skip(si.ebps);
    return r.over ? PARSE : 0;
  }
  if (si.kind == KIND_VERBATIM) {
    r.skip_bits(static_cast<uint64_t>(si.ebps) * bs);
    return r.over ? PARSE : 0;
  }
  r.skip_bits(static_cast<uint64_t>(si.ebps) * si.order);
  if (si.kind == KIND_LPC) {
    const uint32_t prec = r.u(4) + 1;
    const int32_t shift = r.s(5);
    if (prec == 16 || shift < 0) return PARSE;
    r.skip_bits(static_cast<uint64_t>(prec) * si.order);
  }
  if (r.over) return PARSE;
  ResidualState rs;
  if (residual_begin(r, bs, si.order, rs)) return PARSE;
  uint32_t bad = 0;
  for (uint32_t t = si.order; t < bs; ++t) {
    if (residual_partition(r, si.order, rs)) return PARSE;
    if (rs.escaped) {  // a run of fixed-width values: skip it whole
      r.skip_bits(static_cast<uint64_t>(rs.param) * rs.left);
      t += rs.left - 1;
      rs.left = 0;
    } else {
      residual_next(r, rs, &bad);
    }
    if (r.over || bad) return PARSE;
  }
  // a partition 0 without samples (order == block size) still has its header
  while (rs.part < rs.nparts) {
    if (residual_open(r, si.order, rs) || rs.left != 0) return PARSE;
  }
  return r.over ? PARSE : 0;
}

// per-frame record of the skim: 48 bytes
struct FrameRec {
  uint32_t status;
  uint32_t block_size;
  uint32_t info;  // channels | ch_tag << 4 | bps << 8
  uint32_t len;   // parsed length in bytes, CRC-16 included
  uint32_t sub_bit[MAX_CHANNELS];
};

// Header + every subframe's codes.  `len` is the frame's byte span (decode: lengths[f]; index: what is left of the
// buffer).  check_length: LENGTH when the parsed length differs from len.  The CRC-16 is left to the caller.
FD_HD void skim_frame(const uint8_t* p, uint32_t len, uint32_t channels, uint32_t bps, uint32_t max_block_size,
                      uint32_t max_bps, bool check_length, const CrcTables& tab, FrameRec& rec, uint64_t* number) {
  rec.status = 0;
  rec.block_size = 0;
  rec.info = 0;
  rec.len = 0;
  for (uint32_t c = 0; c < MAX_CHANNELS; ++c) rec.sub_bit[c] = 0;
  Header h;
  uint32_t st = parse_header(p, len, channels, bps, max_block_size, max_bps, tab, h);
  if (number) *number = st & (BAD_HEADER | HEADER_CRC) ? 0 : h.number;
  if (st) {
    rec.status = st;
    return;
  }
  BitReader r;
  r.init(p, len, static_cast<uint64_t>(h.header_bytes) * 8);
  for (uint32_t c = 0; c < h.channels; ++c) {
    rec.sub_bit[c] = static_cast<uint32_t>(r.pos());
    if (skim_subframe(r, h.block_size, subframe_bps(h.bps, h.ch_tag, c))) {
      rec.status = PARSE;
      return;
    }
  }
  const uint64_t body = (r.pos() + 7) >> 3;
  const uint64_t parsed = body + 2;
  if (parsed > len) {
    rec.status = check_length ? LENGTH : PARSE;
    return;
  }
  rec.len = static_cast<uint32_t>(parsed);
  if (check_length && parsed != len) {
    rec.status = LENGTH;
    return;
  }
  rec.block_size = h.block_size;
  rec.info = h.channels | (h.ch_tag << 4) | (h.bps << 8);
}

// serial CRC-16 of p[0 .. n)
FD_HD uint32_t crc16(const uint8_t* p, uint32_t n, const CrcTables& tab) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; ++i) c = ((c << 8) & 0xFFFFu) ^ tab.t16[((c >> 8) ^ p[i]) & 0xFFu];
  return c;
}

// ---- reconstruction of one subframe: the last MAXP samples in registers ----
// Predictions accumulate in 64 bits and truncate to i32 (decode_lpc, src/component/decode.rs:159-177 of the
// reference); Fixed orders are LPC with the coefficients of RFC 9639 table 21 and shift 0.  Call init() on a subframe
// that skim_subframe accepted, then next() block-size times.
template <int MAXP>
struct SubDecoder {
  BitReader warm;  // the warm-up samples (Verbatim: every sample)
  BitReader res;   // the residual
  ResidualState rs;
  uint32_t kind, order, wasted, ebps, shift, t, warm_n;
  int32_t cval;
  int32_t coef[MAXP];
  int32_t hist[MAXP];  // hist[0] = the previous sample

  FD_HD void init(const uint8_t* p, uint32_t len, uint32_t start_bit, uint32_t bs, uint32_t sbps) {
    BitReader r;
    r.init(p, len, start_bit);
    SubInfo si;
    parse_subframe_header(r, bs, sbps, si);
    kind = si.kind;
    order = si.order;
    wasted = si.wasted;
    ebps = si.ebps;
    shift = 0;
    t = 0;
    cval = 0;
FD_UNROLL
    for (int j = 0; j < MAXP; ++j) {
      coef[j] = 0;
      hist[j] = 0;
    }
    warm = r;
    warm_n = kind == KIND_VERBATIM ? bs : order;
    if (kind == KIND_CONSTANT) {
      cval = r.s(ebps);
      return;
    }
    if (kind == KIND_VERBATIM) return;
    r.skip_bits(static_cast<uint64_t>(ebps) * order);
    if (kind == KIND_FIXED) {
      // RFC 9639 section 9.2.5, table 21: {1}, {2, -1}, {3, -3, 1}, {4, -6, 4, -1}
      const int32_t o = static_cast<int32_t>(order);
      coef[0] = o;
      if (MAXP > 1) coef[1 % MAXP] = o == 2 ? -1 : o == 3 ? -3 : o == 4 ? -6 : 0;
      if (MAXP > 2) coef[2 % MAXP] = o == 3 ? 1 : o == 4 ? 4 : 0;
      if (MAXP > 3) coef[3 % MAXP] = o == 4 ? -1 : 0;
    } else {
      const uint32_t prec = r.u(4) + 1;
      shift = static_cast<uint32_t>(r.s(5));
FD_UNROLL
      for (int j = 0; j < MAXP; ++j)
        if (static_cast<uint32_t>(j) < order) coef[j] = r.s(prec);
    }
    res = r;
    residual_begin(res, bs, order, rs);
  }

  FD_HD int32_t next() {
    int32_t v;
    if (t < warm_n) {
      v = warm.s(ebps);
    } else if (kind == KIND_CONSTANT) {
      v = cval;
    } else {
      uint32_t bad = 0;
      residual_partition(res, order, rs);
      const int32_t e = residual_next(res, rs, &bad);
      int64_t pred = 0;
FD_UNROLL
      for (int j = 0; j < MAXP; ++j) pred += static_cast<int64_t>(coef[j]) * hist[j];
      v = static_cast<int32_t>(static_cast<uint32_t>(e) + static_cast<uint32_t>(static_cast<int32_t>(pred >> shift)));
    }
FD_UNROLL
    for (int j = MAXP - 1; j > 0; --j) hist[j] = hist[j - 1];
    hist[0] = v;
    ++t;
    return static_cast<int32_t>(static_cast<uint32_t>(v) << wasted);
  }
};

// decode.rs:71-98: undo the stereo decorrelation for one sample pair (a = channel 0, b = channel 1 as decoded)
FD_HD void undo_stereo(uint32_t ch_tag, int32_t& a, int32_t& b) {
  if (ch_tag == 8) {
    b = static_cast<int32_t>(static_cast<uint32_t>(a) - static_cast<uint32_t>(b));
  } else if (ch_tag == 9) {
    a = static_cast<int32_t>(static_cast<uint32_t>(a) + static_cast<uint32_t>(b));
  } else if (ch_tag == 10) {
    const int32_t s = b;
    const int32_t m = static_cast<int32_t>((static_cast<uint32_t>(a) << 1) | static_cast<uint32_t>(s & 1));
    a = static_cast<int32_t>(static_cast<uint32_t>(m) + static_cast<uint32_t>(s)) >> 1;
    b = static_cast<int32_t>(static_cast<uint32_t>(m) - static_cast<uint32_t>(s)) >> 1;
  }
}

// ---- the wide forms: frames of more than WIDE_ABOVE_BPS bits per sample ----
// The side subframe of a 32-bit stereo frame carries 33-bit samples, and undoing mid/side forms (mid << 1 | side & 1)
// +- side, which reaches 34 bits.  The wide decoder therefore keeps its history, its constant and its value in 64 bits:
// the prediction is a sum of at most 32 products of a 15-bit coefficient and a 33-bit sample, below 2^52, and
// e + (pred >> shift) with a 32-bit residual stays below 2^53.  The value rule: on a valid stream every channel value
// behind undo_stereo_wide fits 32 bits, and that int32_t is the result; on an invalid stream that passes both CRCs the
// result is the low 32 bits of the same computation carried out in two's-complement 64-bit arithmetic (sums, products
// and left shifts wrap at 64 bits, right shifts are arithmetic) -- not the narrow decoder's truncation to i32 at every
// step.  Both builds run this one code, so they agree on every input.  Residuals stay int32_t: a valid stream's fit
// (RFC 9639 section 9.2.7.3) and residual_next rejects longer codes.
// WideSubDecoder is SubDecoder line for line but for the value type, s64 in place of s and the 64-bit wrap: the narrow
// one is kept as it was on purpose, so a change to either's parse steps (init, the order of reads in next) goes into
// both.
template <int MAXP>
struct WideSubDecoder {
  BitReader warm;  // the warm-up samples (Verbatim: every sample)
  BitReader res;   // the residual
  ResidualState rs;
  uint32_t kind, order, wasted, ebps, shift, t, warm_n;
  int64_t cval;
  int32_t coef[MAXP];
  int64_t hist[MAXP];  // hist[0] = the previous sample

  FD_HD void init(const uint8_t* p, uint32_t len, uint32_t start_bit, uint32_t bs, uint32_t sbps) {
    BitReader r;
    r.init(p, len, start_bit);
    SubInfo si;
    parse_subframe_header(r, bs, sbps, si);
    kind = si.kind;
    order = si.order;
    wasted = si.wasted;
    ebps = si.ebps;
    shift = 0;
    t = 0;
    cval = 0;
FD_UNROLL
    for (int j = 0; j < MAXP; ++j) {
      coef[j] = 0;
      hist[j] = 0;
    }
    warm = r;
    warm_n = kind == KIND_VERBATIM ? bs : order;
    if (kind == KIND_CONSTANT) {
      cval = r.s64(ebps);
      return;
    }
    if (kind == KIND_VERBATIM) return;
    r.skip_bits(static_cast<uint64_t>(ebps) * order);
    if (kind == KIND_FIXED) {
      const int32_t o = static_cast<int32_t>(order);
      coef[0] = o;
      if (MAXP > 1) coef[1 % MAXP] = o == 2 ? -1 : o == 3 ? -3 : o == 4 ? -6 : 0;
      if (MAXP > 2) coef[2 % MAXP] = o == 3 ? 1 : o == 4 ? 4 : 0;
      if (MAXP > 3) coef[3 % MAXP] = o == 4 ? -1 : 0;
    } else {
      const uint32_t prec = r.u(4) + 1;
      shift = static_cast<uint32_t>(r.s(5));
FD_UNROLL
      for (int j = 0; j < MAXP; ++j)
        if (static_cast<uint32_t>(j) < order) coef[j] = r.s(prec);
    }
    res = r;
    residual_begin(res, bs, order, rs);
  }

  FD_HD int64_t next() {
    int64_t v;
    if (t < warm_n) {
      v = warm.s64(ebps);
    } else if (kind == KIND_CONSTANT) {
      v = cval;
    } else {
      uint32_t bad = 0;
      residual_partition(res, order, rs);
      const int32_t e = residual_next(res, rs, &bad);
      uint64_t pred = 0;  // unsigned: wraps at 64 bits on an invalid stream
FD_UNROLL
      for (int j = 0; j < MAXP; ++j)
        pred += static_cast<uint64_t>(static_cast<int64_t>(coef[j])) * static_cast<uint64_t>(hist[j]);
      v = static_cast<int64_t>(static_cast<uint64_t>(static_cast<int64_t>(e)) +
                               static_cast<uint64_t>(static_cast<int64_t>(pred) >> shift));
    }
FD_UNROLL
    for (int j = MAXP - 1; j > 0; --j) hist[j] = hist[j - 1];
    hist[0] = v;
    ++t;
    return static_cast<int64_t>(static_cast<uint64_t>(v) << wasted);
  }
};

// undo_stereo on the wide decoder's values; the caller keeps the low 32 bits of a and b
FD_HD void undo_stereo_wide(uint32_t ch_tag, int64_t& a, int64_t& b) {
  const uint64_t ua = static_cast<uint64_t>(a), ub = static_cast<uint64_t>(b);
  if (ch_tag == 8) {
    b = static_cast<int64_t>(ua - ub);
  } else if (ch_tag == 9) {
    a = static_cast<int64_t>(ua + ub);
  } else if (ch_tag == 10) {
    const uint64_t m = (ua << 1) | (ub & 1u);
    a = static_cast<int64_t>(m + ub) >> 1;
    b = static_cast<int64_t>(m - ub) >> 1;
  }
}

// the decoder of a frame: Decoder<MAXP, WIDE>::type
template <int MAXP, bool WIDE>
struct Decoder {
  typedef SubDecoder<MAXP> type;
};
template <int MAXP>
struct Decoder<MAXP, true> {
  typedef WideSubDecoder<MAXP> type;
};

// does a frame of `bps` bits per sample take the wide decoder?
FD_HD bool needs_wide(uint32_t bps) { return bps > WIDE_ABOVE_BPS; }

// order bucket of the decoder's register history
FD_HD int order_bucket(uint32_t order) { return order <= 4 ? 4 : order <= 8 ? 8 : order <= 16 ? 16 : 32; }

}  // namespace flacdec

#endif  // FLAC_DECODE_CORE_H_
