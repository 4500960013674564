// rice_escape_core.h -- the per-partition arithmetic of FLACENC_HIP_FLAG_RICE_ESCAPE (rice_escape.cpp's
// rice_escape_kernel), shared by the device kernel, the packers and a host build
// (tests/test_rice_escape_cpu.py compiles this header's own text with g++): the raw width of a partition from its
// extremes, the cost of storing it escaped, the choice between that and the Rice code, and the exact bits a partition
// takes in Residual::write.  Integers only.
#ifndef FLACENC_HIP_RICE_ESCAPE_CORE_H_
#define FLACENC_HIP_RICE_ESCAPE_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define RE_HD __host__ __device__ inline
#else
#define RE_HD inline
#endif

namespace rice_escape {

constexpr uint32_t kMark = 0x80u;       // rice_params[q] = kMark | width: partition q is escaped
constexpr uint32_t kMaxWidth = 31u;     // the 5-bit width field holds 0..31; width 32 cannot be escaped
constexpr uint32_t kNoEscape = 0xFFFFFFFFu;

RE_HD bool is_marked(uint32_t param) { return (param & kMark) != 0u; }
RE_HD uint32_t marked_width(uint32_t param) { return param & 31u; }

// The smallest w with -2^(w-1) <= lo and hi < 2^(w-1) for the extremes lo <= hi of a partition; 0 when both are zero.
// An empty partition is given lo = hi = 0.  Up to 32.
RE_HD uint32_t raw_width(int32_t lo, int32_t hi) {
  // v needs w bits iff v ^ (v >> 31) < 2^(w-1): the magnitude bits of v (of ~v when negative), plus the sign
  const uint32_t m = ((uint32_t)lo ^ (uint32_t)(lo >> 31)) | ((uint32_t)hi ^ (uint32_t)(hi >> 31));
  if (lo == 0 && hi == 0) return 0u;
  uint32_t bits = 0;
  for (uint32_t x = m; x != 0u; x >>= 1) ++bits;
  return bits + 1u;
}

// E = 4 + 5 + cnt * w, the partition's cost beside the Rice table's (which counts a 4-bit parameter);
// kNoEscape when the width does not fit the field.  cnt <= 32767, so E < 2^20.
RE_HD uint32_t escape_cost(uint32_t cnt, uint32_t width) {
  return width <= kMaxWidth ? 9u + cnt * width : kNoEscape;
}

// Escaped iff E < R, strictly: a tie stays Rice.
RE_HD bool choose_escape(uint32_t rice_cost, uint32_t esc_cost) { return esc_cost < rice_cost; }

// The byte the record holds for a partition, and the cost the level's sum takes
RE_HD uint32_t chosen_param(uint32_t rice_cost, uint32_t rice_param, uint32_t cnt, uint32_t width) {
  return choose_escape(rice_cost, escape_cost(cnt, width)) ? (kMark | width) : rice_param;
}
RE_HD uint32_t chosen_cost(uint32_t rice_cost, uint32_t cnt, uint32_t width) {
  const uint32_t e = escape_cost(cnt, width);
  return choose_escape(rice_cost, e) ? e : rice_cost;
}

// The bits of one partition in Residual::write without its parameter field: 5 + cnt * w escaped, else the quotients'
// unary bits, the stop bits and the remainders
RE_HD uint64_t partition_body_bits(uint32_t param, uint32_t cnt, uint64_t sum_quotients) {
  if (is_marked(param)) return 5u + (uint64_t)cnt * marked_width(param);
  return sum_quotients + (uint64_t)cnt * (param + 1u);
}

// 5-bit parameters exactly when a NON-escaped parameter exceeds 14
RE_HD bool wants_rice2(uint32_t param) { return !is_marked(param) && param > 14u; }

}  // namespace rice_escape
#endif
