// wide_encode_core.h -- the wide encode path (flacenc_hip_encode_pack_frames_wide): the
// whole rule and a serial frame writer in plain C++.  Samples of 8..32 bits, a 33-bit side channel; Constant, Verbatim
// and the fixed predictors of order 0..4 with the exhaustive partitioned-Rice search, wasted bits, the stereo decision.
// No floating point and no 32-bit difference: a role's sample and every difference are int64, a residual that is coded
// lies in (-2^31, 2^31) (RFC 9639 section 9.2.7.3), so its zigzag form is a uint32 and every sum of them a uint64.
// Shared by the kernels (wide_encode.cpp) and a host build (tests/host/wide_encode_core_test.cpp, under the sanitizers);
// both are held to tests/wide_model.py byte for byte.
#ifndef WIDE_ENCODE_CORE_H_
#define WIDE_ENCODE_CORE_H_

#include <stdint.h>
#include <stddef.h>

#include "variable_block_core.h"

namespace wideenc {

constexpr uint32_t MAX_PARTS = 256;      // 2^8: a block below 2^15 samples has at most 511 runs of 64
constexpr uint32_t MAX_PARAMS = 31;      // parameters 0..=30
constexpr uint32_t LOW_PARAMS = 15;      // sums of u >> p for p < 15 are uint64, for p >= 15 uint32 (see Tables)
constexpr uint32_t MIN_PREDICTION = 64;  // MIN_BLOCK_SIZE_FOR_PREDICTION, coding.rs:396
enum : uint8_t { KIND_CONSTANT = 0, KIND_VERBATIM = 1, KIND_FIXED = 2 };

struct Config {  // what the path reads of a flacenc_hip_frame_config
  uint32_t use_constant, use_fixed, fixed_max_order, max_rice_parameter;
  uint32_t use_leftside, use_rightside, use_midside, wasted_bits;
};

// encode_subframe's answer for one role of one frame
struct SubRecord {
  uint8_t kind, k, order, porder;  // k: wasted bits; order, porder, params: KIND_FIXED only
  uint32_t five;                   // 1: a parameter exceeds 14, the residual is RICE2 (5-bit parameters)
  int64_t value;                   // KIND_CONSTANT: the sample
  uint64_t bits;                   // SubFrame::count_bits + k
  uint8_t params[MAX_PARTS];
};

struct Rows {  // a frame's channel rows
  const int32_t* x;
  size_t stride;
  uint32_t channels;
};

FD_HD uint32_t roles_of(uint32_t channels) { return channels == 2 ? 4u : channels; }
FD_HD uint32_t role_width(uint32_t channels, uint32_t role, uint32_t bits) { return bits + ((channels == 2 && role == 3) ? 1u : 0u); }

// sample t of a role: L, R, M = (L + R) >> 1, S = L - R of a 2-channel frame (coding.rs:476-484), else channel `role`
FD_HD int64_t role_sample(const Rows& r, uint32_t role, uint32_t t) {
  if (r.channels != 2) return r.x[role * r.stride + t];
  const int64_t a = r.x[t], b = r.x[r.stride + t];
  return role == 0 ? a : role == 1 ? b : role == 2 ? ((a + b) >> 1) : (a - b);
}

// the o-th difference at t >= o of the role's samples >> k
FD_HD int64_t fixed_error(const Rows& r, uint32_t role, uint32_t k, uint32_t o, uint32_t t) {
  const int64_t x0 = role_sample(r, role, t) >> k;
  if (o == 0) return x0;
  const int64_t x1 = role_sample(r, role, t - 1) >> k;
  if (o == 1) return x0 - x1;
  const int64_t x2 = role_sample(r, role, t - 2) >> k;
  if (o == 2) return x0 - 2 * x1 + x2;
  const int64_t x3 = role_sample(r, role, t - 3) >> k;
  if (o == 3) return x0 - 3 * x1 + 3 * x2 - x3;
  const int64_t x4 = role_sample(r, role, t - 4) >> k;
  return x0 - 4 * x1 + 6 * x2 - 4 * x3 + x4;
}

FD_HD bool codable(int64_t e) { return e > -(1ll << 31) && e < (1ll << 31); }
FD_HD uint32_t zigzag(int64_t e) { return e < 0 ? static_cast<uint32_t>(-2 * e - 1) : static_cast<uint32_t>(2 * e); }

// finest_partition_order, rice.rs:157-165, with min_part_size = max(64, o) = 64 for o <= 4
FD_HD uint32_t finest_order(uint32_t n) {
  const uint32_t splits = n / MIN_PREDICTION;
  if (splits == 0) return 0;
  uint32_t lg = 0, tz = 0;
  while ((splits >> (lg + 1)) != 0) ++lg;
  while (((n >> tz) & 1u) == 0) ++tz;
  const uint32_t m = lg < tz ? lg : tz;
  return m < 15 ? m : 15;
}

FD_HD uint32_t wasted_of(uint64_t or_all, bool constant, const Config& c) {
  if (!c.wasted_bits || or_all == 0 || (c.use_constant && constant)) return 0;
  uint32_t k = 0;
  while (((or_all >> k) & 1u) == 0) ++k;
  return k;
}

// The sums of one fixed order at the finest partition order F: lo[q][p] = sum of u >> p over partition q for p < 15,
// hi[q][p - 15] for p >= 15.  A block has fewer than 2^15 samples and u >> 15 < 2^17: a sum of them over any set of
// samples of one block is below 2^32, at every level of the merge; the low parameters need 47 bits.
struct Tables {
  unsigned long long lo[MAX_PARTS][LOW_PARAMS];
  uint32_t hi[MAX_PARTS][MAX_PARAMS - LOW_PARAMS];
};
FD_HD unsigned long long table_sum(const Tables& t, uint32_t q, uint32_t p) {
  return p < LOW_PARAMS ? t.lo[q][p] : t.hi[q][p - LOW_PARAMS];
}

// PrcBitTable::minimizer for a partition of `count` coded samples: the smallest 4 + count (p + 1) + sum, ties to the
// lowest p
FD_HD unsigned long long best_parameter(const Tables& t, uint32_t q, uint32_t count, uint32_t max_p, uint32_t* p_out) {
  unsigned long long best = ~0ull;
  uint32_t bp = 0;
  for (uint32_t p = 0; p <= max_p; ++p) {
    const unsigned long long bits = 4ull + static_cast<unsigned long long>(count) * (p + 1) + table_sum(t, q, p);
    if (bits < best) {
      best = bits;
      bp = p;
    }
  }
  *p_out = bp;
  return best;
}

// level `level`'s partition j lives at finest index j << (F - level): merging adds the odd neighbour into the even one
FD_HD void merge_pair(Tables& t, uint32_t even, uint32_t odd, uint32_t p) {
  if (p < LOW_PARAMS) t.lo[even][p] += t.lo[odd][p];
  else t.hi[even][p - LOW_PARAMS] += t.hi[odd][p - LOW_PARAMS];
}

struct Choice {  // the best (order, partition order, parameters) so far
  bool have;
  unsigned long long key, code_bits;
  uint32_t order, porder;
  uint8_t params[MAX_PARTS];
};

// encode_subframe's last step (coding.rs:403-416 without the LPC candidate) from the best fixed candidate: `have`, its
// key, code_bits, order, partition order and parameters
FD_HD void finish_record(bool have, unsigned long long key, unsigned long long code_bits, uint32_t order, uint32_t porder,
                         const uint8_t* params, uint32_t n, uint32_t w, uint32_t k, SubRecord* out) {
  const unsigned long long verbatim_bits = 8ull + static_cast<unsigned long long>(n) * w;
  out->kind = KIND_VERBATIM;
  out->k = static_cast<uint8_t>(k);
  out->order = out->porder = 0;
  out->five = 0;
  out->value = 0;
  out->bits = verbatim_bits + k;
  if (!have || key >= verbatim_bits) return;
  uint32_t five = 0;
  for (uint32_t q = 0; q < (1u << porder); ++q) five |= params[q] > 14 ? 1u : 0u;
  const unsigned long long count_bits =
      8ull + static_cast<unsigned long long>(w) * order + 6ull + code_bits + (five ? (1ull << porder) : 0ull);
  if (count_bits >= verbatim_bits) return;
  out->kind = KIND_FIXED;
  out->order = static_cast<uint8_t>(order);
  out->porder = static_cast<uint8_t>(porder);
  out->five = five;
  out->bits = count_bits + k;
  for (uint32_t q = 0; q < (1u << porder); ++q) out->params[q] = params[q];
}

FD_HD void constant_record(int64_t value, uint32_t width, SubRecord* out) {
  out->kind = KIND_CONSTANT;
  out->k = out->order = out->porder = 0;
  out->five = 0;
  out->value = value;
  out->bits = 8ull + width;  // bitrepr.rs:445
}

// try_stereo_coding, coding.rs:493-522 -> the channel tag of the header; roles[] the two subframes' roles
FD_HD uint32_t stereo_choice(const unsigned long long bits[4], const Config& c, uint32_t roles[2]) {
  unsigned long long best = bits[0] + bits[1];
  uint32_t tag = 1;
  roles[0] = 0;
  roles[1] = 1;
  if (c.use_leftside && bits[0] + bits[3] < best) {
    best = bits[0] + bits[3];
    tag = 8;
    roles[0] = 0;
    roles[1] = 3;
  }
  if (c.use_rightside && bits[1] + bits[3] < best) {
    best = bits[1] + bits[3];
    tag = 9;
    roles[0] = 3;
    roles[1] = 1;
  }
  if (c.use_midside && bits[2] + bits[3] < best) {
    tag = 10;
    roles[0] = 2;
    roles[1] = 3;
  }
  return tag;
}

// The frame header as the packers write it (fill_header_specs, api_pack.cpp), with sample-size code 7 for 32 bits and 0
// for the depths that have no code.  `out` has room for 16 bytes; returns the length.
FD_HD uint32_t write_header(uint32_t block_size, uint32_t sample_rate, uint32_t bits, uint32_t tag, uint32_t number,
                            uint8_t* out) {
  uint32_t bs_tag = 0, extra_len = 0;
  uint8_t extra[4] = {0, 0, 0, 0};
  if (block_size == 192) bs_tag = 1;
  for (uint32_t x = 0; x < 4 && !bs_tag; ++x)
    if (block_size == (576u << x)) bs_tag = 2 + x;
  for (uint32_t x = 0; x < 8 && !bs_tag; ++x)
    if (block_size == (256u << x)) bs_tag = 8 + x;
  if (!bs_tag) {
    if (block_size <= 256) {
      bs_tag = 6;
      extra[extra_len++] = static_cast<uint8_t>(block_size - 1);
    } else {
      bs_tag = 7;
      extra[extra_len++] = static_cast<uint8_t>((block_size - 1) >> 8);
      extra[extra_len++] = static_cast<uint8_t>(block_size - 1);
    }
  }
  const uint32_t known[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  uint32_t sr_tag = 0;
  for (uint32_t t = 1; t < 12; ++t)
    if (sample_rate == known[t]) sr_tag = t;
  if (!sr_tag && sample_rate) {
    if (sample_rate % 1000 == 0 && sample_rate / 1000 <= 255) {
      sr_tag = 12;
      extra[extra_len++] = static_cast<uint8_t>(sample_rate / 1000);
    } else if (sample_rate % 10 == 0 && sample_rate / 10 <= 65535) {
      sr_tag = 14;
      extra[extra_len++] = static_cast<uint8_t>((sample_rate / 10) >> 8);
      extra[extra_len++] = static_cast<uint8_t>(sample_rate / 10);
    } else if (sample_rate <= 65535) {
      sr_tag = 13;
      extra[extra_len++] = static_cast<uint8_t>(sample_rate >> 8);
      extra[extra_len++] = static_cast<uint8_t>(sample_rate);
    }
  }
  const uint32_t ss_tag = bits == 8 ? 1u : bits == 12 ? 2u : bits == 16 ? 4u : bits == 20 ? 5u : bits == 24 ? 6u : bits == 32 ? 7u : 0u;
  out[0] = 0xFF;
  out[1] = 0xF8;
  out[2] = static_cast<uint8_t>((bs_tag << 4) | sr_tag);
  out[3] = static_cast<uint8_t>((tag << 4) | (ss_tag << 1));
  uint32_t at = 4 + vbs::write_coded_number(out + 4, number);
  for (uint32_t i = 0; i < extra_len; ++i) out[at++] = extra[i];
  out[at] = static_cast<uint8_t>(vbs::crc8_bytes(out, at));
  return at + 1;
}

// `nbits` <= 33 bits of v at bit `pos` (0 = the first byte's top bit) of a zeroed buffer of big-endian bytes held in
// 4-byte aligned words: the field lies in two words at most.  Or::operator()(uint32_t* word, uint32_t bits_in_memory).
template <typename Or>
FD_HD void put_bits(uint32_t* words, uint64_t pos, uint64_t v, uint32_t nbits, Or word_or) {
  if (nbits == 0) return;
  const uint32_t sh = static_cast<uint32_t>(pos & 31u);
  v &= nbits >= 64 ? ~0ull : ((1ull << nbits) - 1ull);
  const uint64_t window = v << (64u - sh - nbits);  // sh + nbits <= 31 + 33
  const uint32_t first = static_cast<uint32_t>(window >> 32), second = static_cast<uint32_t>(window);
  uint32_t* w = words + (pos >> 5);
  if (first) word_or(w, __builtin_bswap32(first));
  if (second) word_or(w + 1, __builtin_bswap32(second));
}

// bits a subframe spends before its samples: the type byte and the unary k
FD_HD uint32_t subframe_head_bits(uint32_t k) { return 8u + k; }

template <typename Or>
FD_HD void put_subframe_head(uint32_t* words, uint64_t pos, const SubRecord& rec, Or word_or) {
  const uint32_t type = rec.kind == KIND_CONSTANT ? 0u : rec.kind == KIND_VERBATIM ? 1u : 8u + rec.order;
  put_bits(words, pos, (type << 1) | (rec.k ? 1u : 0u), 8, word_or);
  if (rec.k) put_bits(words, pos + 8, 1, rec.k, word_or);  // k - 1 zeros and a one
}

// bits of the coded sample t (>= order) of a Fixed subframe, the parameter field in front of a partition's first
// sample included; *param_bits gets that field's width (0 inside a partition)
FD_HD uint32_t code_length(const SubRecord& rec, uint32_t n, uint32_t t, uint32_t u, uint32_t* param_out,
                           uint32_t* param_bits) {
  const uint32_t size = n >> rec.porder, q = t / size;
  const uint32_t p = rec.params[q];
  const uint32_t start = q == 0 ? rec.order : q * size;
  *param_out = p;
  *param_bits = t == start ? (rec.five ? 5u : 4u) : 0u;
  return *param_bits + (u >> p) + 1u + p;
}

struct PlainOr {
#if defined(__HIPCC__)
  __host__ __device__
#endif
  void operator()(uint32_t* w, uint32_t v) const { *w |= v; }
};

#ifndef __HIP_DEVICE_COMPILE__
// ---------------------------------------------------------------- the serial statement (host)
// encode_subframe for one role (section 4.29's rule, tests/wide_model.py)
inline void decide_role(const Rows& r, uint32_t role, uint32_t n, uint32_t width, const Config& c, Tables* tab,
                        SubRecord* out) {
  uint64_t or_all = 0;
  bool constant = true;
  const int64_t first = role_sample(r, role, 0);
  for (uint32_t t = 0; t < n; ++t) {
    const int64_t v = role_sample(r, role, t);
    or_all |= static_cast<uint64_t>(v);
    constant = constant && v == first;
  }
  for (uint32_t q = 0; q < MAX_PARTS; ++q) out->params[q] = 0;
  if (c.use_constant && constant) {
    constant_record(first, width, out);
    return;
  }
  const uint32_t k = wasted_of(or_all, constant, c), w = width - k;
  Choice best{};
  Choice cur{};
  const uint32_t max_order = c.fixed_max_order < 4 ? c.fixed_max_order : 4;
  const uint32_t F = finest_order(n), size = n >> F;
  for (uint32_t o = 0; n >= MIN_PREDICTION && c.use_fixed && o <= max_order; ++o) {
    bool ok = true;
    for (uint32_t q = 0; q < (1u << F); ++q) {
      for (uint32_t p = 0; p < LOW_PARAMS; ++p) tab->lo[q][p] = 0;
      for (uint32_t p = LOW_PARAMS; p < MAX_PARAMS; ++p) tab->hi[q][p - LOW_PARAMS] = 0;
    }
    for (uint32_t t = o; t < n && ok; ++t) {
      const int64_t e = fixed_error(r, role, k, o, t);
      ok = codable(e);
      if (!ok) break;
      const uint32_t u = zigzag(e), q = t / size;
      for (uint32_t p = 0; p < LOW_PARAMS; ++p) tab->lo[q][p] += u >> p;
      for (uint32_t p = LOW_PARAMS; p < MAX_PARAMS; ++p) tab->hi[q][p - LOW_PARAMS] += u >> p;
    }
    if (!ok) continue;
    for (uint32_t level = F;; --level) {
      const uint32_t parts = 1u << level, step = 1u << (F - level);
      unsigned long long total = 0;
      uint8_t ps[MAX_PARTS];
      for (uint32_t j = 0; j < parts; ++j) {
        uint32_t p;
        total += best_parameter(*tab, j * step, (n >> level) - (j == 0 ? o : 0), c.max_rice_parameter, &p);
        ps[j] = static_cast<uint8_t>(p);
      }
      if (level == F || total < cur.code_bits) {
        cur.code_bits = total;
        cur.porder = level;
        for (uint32_t j = 0; j < parts; ++j) cur.params[j] = ps[j];
      }
      if (level == 0) break;
      for (uint32_t j = 0; j < parts / 2; ++j)
        for (uint32_t p = 0; p < MAX_PARAMS; ++p) merge_pair(*tab, 2 * j * step, (2 * j + 1) * step, p);
    }
    cur.key = static_cast<unsigned long long>(w) * o + cur.code_bits;
    if (!best.have || cur.key < best.key) {
      best = cur;
      best.have = true;
      best.order = o;
    }
  }
  finish_record(best.have, best.key, best.code_bits, best.order, best.porder, best.params, n, w, k, out);
}

// One frame, serially: the roles' records, the stereo decision, the header, the subframes, the CRC-16.  `out` is
// 4-byte aligned with room for the frame's bytes bound rounded up to 16; returns the length.
inline uint32_t write_frame(const Rows& r, uint32_t n, uint32_t bits, uint32_t sample_rate, uint32_t number,
                            const Config& c, Tables* tab, SubRecord* recs, uint8_t* out, size_t room) {
  const uint32_t roles = roles_of(r.channels);
  for (uint32_t role = 0; role < roles; ++role) decide_role(r, role, n, role_width(r.channels, role, bits), c, tab, recs + role);
  uint32_t chosen[8], tag = r.channels - 1;
  for (uint32_t ch = 0; ch < r.channels; ++ch) chosen[ch] = ch;
  if (r.channels == 2) {
    const unsigned long long b[4] = {recs[0].bits, recs[1].bits, recs[2].bits, recs[3].bits};
    tag = stereo_choice(b, c, chosen);
  }
  for (size_t i = 0; i < room; ++i) out[i] = 0;
  uint32_t* words = reinterpret_cast<uint32_t*>(out);
  uint64_t pos = 8ull * write_header(n, sample_rate, bits, tag, number, out);
  const PlainOr por;
  for (uint32_t ch = 0; ch < r.channels; ++ch) {
    const SubRecord& rec = recs[chosen[ch]];
    const uint32_t role = chosen[ch], w = role_width(r.channels, role, bits) - rec.k;
    put_subframe_head(words, pos, rec, por);
    uint64_t at = pos + subframe_head_bits(rec.k);
    if (rec.kind == KIND_CONSTANT) {
      put_bits(words, at, static_cast<uint64_t>(rec.value), w, por);
      at += w;
    } else {
      const uint32_t warm = rec.kind == KIND_FIXED ? rec.order : n;
      for (uint32_t t = 0; t < warm; ++t, at += w)
        put_bits(words, at, static_cast<uint64_t>(role_sample(r, role, t) >> rec.k), w, por);
      if (rec.kind == KIND_FIXED) {
        put_bits(words, at, (static_cast<uint64_t>(rec.five) << 4) | rec.porder, 6, por);
        at += 6;
        for (uint32_t t = rec.order; t < n; ++t) {
          const uint32_t u = zigzag(fixed_error(r, role, rec.k, rec.order, t));
          uint32_t p, pb;
          const uint32_t len = code_length(rec, n, t, u, &p, &pb);
          put_bits(words, at, p, pb, por);
          put_bits(words, at + len - p - 1, (1ull << p) | (u & ((1u << p) - 1u)), p + 1, por);
          at += len;
        }
      }
    }
    pos += rec.bits;
    if (at != pos) return 0;  // the counted bits are the written bits
  }
  const uint32_t body = static_cast<uint32_t>((pos + 7) / 8);
  const uint32_t crc = vbs::crc16_bytes(out, body);
  out[body] = static_cast<uint8_t>(crc >> 8);
  out[body + 1] = static_cast<uint8_t>(crc);
  return body + 2;
}
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace wideenc
#endif  // WIDE_ENCODE_CORE_H_
