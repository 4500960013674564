// order_mode_core.h -- the order mode of the certified shapes by material (launch_adaptive, api_candidates.cpp), as a pure
// step over its state, shared with a host build (tests/host/order_mode_core_test.cpp, compiled by g++).
// The certified shapes are blocks of 4096 / 4608 samples at orders up to 12.  The fused kernel settles a subframe's order
// certificate in its first tier for next to nothing; the second tier and the recomputation from the reference's chains are
// serial work of one wave while its workgroup waits -- rare on noise-like material (2 subframes in 393 216 of the bench
// signal), the rule on music (the reference's real-audio fixtures: 26 % / 82 % / 100 % of the subframes at orders
// 8 / 10 / 12 count as unsettled, 220 / 146 / 100 G samples/s where the bench signal runs at 350).  Two passes -- the
// reference's chains on the matrix cores for every subframe, then the fused kernel on their R[] -- give the SAME integers
// at a flat 1.4 x the certified kernel's best time.  So launches that return integers only (no R[], no coefficients: their
// bits depend on the pass that produced them) watch the certificate's counters and take the two-pass form while the
// material they were last given was hard: above kHardShare of the subframes unsettled by the first tier, for a span of
// launches that doubles (8 .. 64) while the probes between the spans keep finding it so.
#ifndef FLACENC_HIP_ORDER_MODE_CORE_H_
#define FLACENC_HIP_ORDER_MODE_CORE_H_

#include <stdint.h>

namespace order_mode {

constexpr double kHardShare = 0.10;
// a verdict is taken from at least this many subframes (counters of smaller launches add up until they are), a probe's from
// at least kProbeMinSubframes; launches of 2^25 subframes and more are not watched (the verdict's fields are 26 bits wide)
constexpr uint32_t kFeedbackMinSubframes = 4096, kProbeMinSubframes = 1024, kFeedbackMaxSubframes = 1u << 25;
constexpr int kFirstSpan = 8, kMaxSpan = 64;

inline uint32_t next_seq(uint32_t seq) { return ((seq + 1u) & 0xFFFu) ? ((seq + 1u) & 0xFFFu) : 1u; }  // (0: the word's initial state)

struct State {
  uint32_t seq = 0, seen_seq = 0, probe_seq = 0;  // sequence numbers of the launches that carried the counters
  uint32_t pending = 0;                           // subframes counted on the device since the last verdict went out
  bool probe_out = false;
  int left = 0, span = 0;                         // two-pass launches left in the span; the span (0: easy material)
};

struct Step {
  bool two_pass;      // the reference's chains in front, no certificate; else the certified kernel
  bool carry;         // the certified launch carries the counters
  uint32_t feedback;  // sequence number of the feedback kernel to send behind it; 0: none
};

// One launch of `n_subframes`, `word` being the latest verdict that has landed (late is fine).  The host may run many
// launches ahead of the device, so nothing is concluded from launches whose counters are not in: on easy material every
// launch carries the counters and any new verdict counts; on hard material a span of two-pass launches is followed by ONE
// probe (a certified launch), and the launches behind the probe stay two-pass until ITS verdict is in.
inline Step step(State& s, uint64_t word, uint32_t n_subframes) {
  if (n_subframes >= kFeedbackMaxSubframes) return {false, false, 0u};
  const uint32_t l_seq = (uint32_t)(word >> 52), l_hard = (uint32_t)(word >> 26) & 0x3FFFFFFu, l_an = (uint32_t)word & 0x3FFFFFFu;
  const bool is_hard = l_an != 0u && (double)l_hard > kHardShare * (double)l_an;
  bool two_pass;
  if (s.span == 0) {  // easy so far
    if (l_seq != s.seen_seq) {
      s.seen_seq = l_seq;
      if (is_hard) s.left = s.span = kFirstSpan;
    }
    two_pass = s.span != 0;
  } else if (s.left > 0) {
    two_pass = true;
  } else if (!s.probe_out) {
    two_pass = false;  // the probe: certified launches until kProbeMinSubframes have been counted
    s.probe_out = true;
    s.probe_seq = 0u;  // (assigned when its feedback goes out)
  } else if (s.probe_seq == 0u) {
    two_pass = false;  // the probe is still collecting
  } else if (l_seq != s.probe_seq) {
    two_pass = true;  // the probe's verdict is not in yet
  } else {
    s.probe_out = false;
    s.seen_seq = l_seq;
    s.span = !is_hard ? 0 : (s.span >= kMaxSpan ? kMaxSpan : 2 * s.span);
    s.left = s.span;
    two_pass = is_hard;
  }
  if (two_pass) {
    if (s.left > 0) --s.left;
    return {true, false, 0u};
  }
  s.pending += n_subframes;
  const bool probing = s.probe_out && s.probe_seq == 0u;
  if (s.pending < (probing ? kProbeMinSubframes : kFeedbackMinSubframes)) return {false, true, 0u};
  s.pending = 0;
  s.seq = next_seq(s.seq);
  if (probing) s.probe_seq = s.seq;
  return {false, true, s.seq};
}

}  // namespace order_mode
#endif
