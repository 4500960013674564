// order_mode_core_test.cpp -- the order mode of the certified shapes (flacenc_rs_amd/csrc/order_mode_core.h) on the CPU:
// scripted verdict sequences against order_mode::step, every expectation stated from the header's constants.  Plain C++
// (g++, once with -O2 and once under ASan + UBSan: tests/test_order_mode_cpu.py).  Exits 0, or prints what failed.
#include <cstdio>

#include "order_mode_core.h"

using namespace order_mode;

namespace {

int g_failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      ++g_failures;                                                  \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    }                                                                \
  } while (0)

constexpr uint32_t kLaunch = kFeedbackMinSubframes;  // a launch that alone fills a verdict
// the verdict word as cert_feedback_kernel (api_candidates.cpp) stores it
uint64_t verdict_word(uint32_t seq, uint64_t hard, uint64_t analysed) {
  return ((uint64_t)(seq & 0xFFFu) << 52) | ((hard & 0x3FFFFFFull) << 26) | (analysed & 0x3FFFFFFull);
}
// a verdict over `analysed` subframes with a share of hard ones just above / well below kHardShare
uint64_t hard_word(uint32_t seq, uint32_t analysed = kLaunch) {
  return verdict_word(seq, (uint64_t)(kHardShare * analysed) + 1, analysed);
}
uint64_t easy_word(uint32_t seq, uint32_t analysed = kLaunch) { return verdict_word(seq, (uint64_t)(kHardShare * analysed), analysed); }

// runs launches until the state is hard with a span of kFirstSpan; returns the verdict word that did it
uint64_t make_hard(State& s) {
  const Step a = step(s, 0, kLaunch);
  CHECK(!a.two_pass && a.carry && a.feedback == 1u);
  const uint64_t word = hard_word(a.feedback);
  const Step b = step(s, word, kLaunch);
  CHECK(b.two_pass && !b.carry && b.feedback == 0u);
  CHECK(s.span == kFirstSpan && s.left == kFirstSpan - 1);
  return word;
}

void easy_material_never_leaves_the_certified_form() {
  State s;
  uint64_t word = 0;
  for (int i = 0; i < 10000; ++i) {
    const Step st = step(s, word, kLaunch);
    CHECK(!st.two_pass && st.carry && st.feedback != 0u);
    CHECK(s.span == 0 && s.left == 0 && !s.probe_out);
    if (i % 3 == 0) word = easy_word(st.feedback);  // (verdicts land late, and exactly at kHardShare is not hard)
  }
  // no verdict at all (analysed == 0) is not hard either
  State t;
  CHECK(!step(t, verdict_word(7, 5, 0), kLaunch).two_pass && t.span == 0);
}

void small_launches_add_up_to_a_verdict() {
  State s;
  const uint32_t n = 1000;
  uint32_t sent = 0, counted = 0;
  for (int i = 0; i < 64; ++i) {
    const Step st = step(s, 0, n);
    counted += n;
    CHECK(!st.two_pass && st.carry);
    CHECK((st.feedback != 0u) == (counted >= kFeedbackMinSubframes));
    if (st.feedback) {
      CHECK(st.feedback == ++sent);
      counted = 0;
    }
  }
  CHECK(sent == 64 / ((kFeedbackMinSubframes + n - 1) / n));
}

void a_hard_verdict_opens_spans_that_double_with_one_probe_each() {
  State s;
  uint64_t word = make_hard(s);
  for (int span = kFirstSpan; ; span = span >= kMaxSpan ? kMaxSpan : 2 * span) {
    CHECK(s.span == span);
    // the rest of the span: two-pass, whatever verdict is read
    while (s.left > 0) {
      const Step st = step(s, word, kLaunch);
      CHECK(st.two_pass && !st.carry && st.feedback == 0u);
    }
    // exactly one probe: certified launches until kProbeMinSubframes are counted, then its feedback
    uint32_t probe_seq = 0, counted = 0, probes = 0;
    while (probe_seq == 0) {
      const Step st = step(s, word, 300);
      counted += 300;
      ++probes;
      CHECK(!st.two_pass && st.carry && s.probe_out);
      CHECK((st.feedback != 0u) == (counted >= kProbeMinSubframes));
      probe_seq = st.feedback;
    }
    CHECK(probes == (kProbeMinSubframes + 299) / 300 && s.probe_seq == probe_seq);
    // launches behind the unanswered probe stay two-pass and send nothing
    for (int i = 0; i < 100; ++i) {
      const Step st = step(s, word, kLaunch);
      CHECK(st.two_pass && !st.carry && st.feedback == 0u && s.span == span && s.left == 0);
    }
    if (span == kMaxSpan && s.seq > 20) break;  // (64 stays 64: seen below a few times)
    word = hard_word(probe_seq, counted);
    const Step st = step(s, word, kLaunch);  // the probe's verdict: still hard, the next span
    const int next = span >= kMaxSpan ? kMaxSpan : 2 * span;
    CHECK(st.two_pass && !s.probe_out && s.span == next && s.left == next - 1);
  }
  CHECK(kFirstSpan == 8 && kMaxSpan == 64);  // 8 -> 16 -> 32 -> 64
}

void an_easy_probe_returns_to_certified() {
  State s;
  const uint64_t word = make_hard(s);
  while (s.left > 0) step(s, word, kLaunch);
  const Step probe = step(s, word, kProbeMinSubframes);
  CHECK(!probe.two_pass && probe.carry && probe.feedback != 0u);
  CHECK(step(s, word, kLaunch).two_pass);  // not in yet
  const Step back = step(s, easy_word(probe.feedback, kProbeMinSubframes), kLaunch);
  CHECK(!back.two_pass && back.carry && s.span == 0 && s.left == 0 && !s.probe_out);
  // ... and that verdict, already seen, is not read again as news
  CHECK(!step(s, hard_word(probe.feedback), kLaunch).two_pass && s.span == 0);
}

void sequence_numbers_wrap_without_zero() {
  CHECK(next_seq(0) == 1u && next_seq(0xFFEu) == 0xFFFu && next_seq(0xFFFu) == 1u);
  State s;
  uint32_t last = 0;
  for (int i = 0; i < 3 * 0x1000; ++i) {
    const Step st = step(s, 0, kLaunch);
    CHECK(st.feedback != 0u && st.feedback <= 0xFFFu && st.feedback == next_seq(last));
    last = st.feedback;
  }
  CHECK((verdict_word(0xFFFu, 0x3FFFFFFu, 0x3FFFFFFu) >> 52) == 0xFFFu);
}

void a_launch_of_2_to_the_25_is_not_watched() {
  State s;
  const Step st = step(s, hard_word(3), kFeedbackMaxSubframes);
  CHECK(!st.two_pass && !st.carry && st.feedback == 0u);
  CHECK(s.seq == 0 && s.seen_seq == 0 && s.pending == 0 && s.span == 0 && s.left == 0 && !s.probe_out);
  CHECK(step(s, 0, kFeedbackMaxSubframes - 1).carry);
  CHECK(kFeedbackMaxSubframes == 1u << 25);
}

}  // namespace

int main() {
  easy_material_never_leaves_the_certified_form();
  small_launches_add_up_to_a_verdict();
  a_hard_verdict_opens_spans_that_double_with_one_probe_each();
  an_easy_probe_returns_to_certified();
  sequence_numbers_wrap_without_zero();
  a_launch_of_2_to_the_25_is_not_watched();
  if (g_failures) fprintf(stderr, "%d checks failed\n", g_failures);
  else puts("order_mode_core: all checks passed");
  return g_failures ? 1 : 0;
}
