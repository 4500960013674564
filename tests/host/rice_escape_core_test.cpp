// Host build of flacenc_rs_amd/csrc/rice_escape_core.h for tests/test_rice_escape_cpu.py: reads one partition per line
// ("lo hi cnt rice_cost rice_param") and prints what the header makes of it ("width escape_cost param cost body_bits
// rice2"; body_bits with the line's sum of quotients taken as rice_cost - 4 - cnt * (rice_param + 1)).  The Python side
// holds every line to tests/escape_model.py.
#include <cinttypes>
#include <cstdio>

#include "rice_escape_core.h"

int main() {
  long long lo, hi;
  unsigned cnt, rice_cost, rice_param;
  while (std::scanf("%lld %lld %u %u %u", &lo, &hi, &cnt, &rice_cost, &rice_param) == 5) {
    const uint32_t w = rice_escape::raw_width((int32_t)lo, (int32_t)hi);
    const uint32_t e = rice_escape::escape_cost(cnt, w);
    const uint32_t par = rice_escape::chosen_param(rice_cost, rice_param, cnt, w);
    const uint32_t cost = rice_escape::chosen_cost(rice_cost, cnt, w);
    const uint64_t sq = (uint64_t)rice_cost - 4u - (uint64_t)cnt * (rice_param + 1u);
    std::printf("%u %" PRId64 " %u %u %" PRIu64 " %d\n", w, e == rice_escape::kNoEscape ? (int64_t)-1 : (int64_t)e, par,
                cost, rice_escape::partition_body_bits(par, cnt, sq), rice_escape::wants_rice2(par) ? 1 : 0);
  }
  return 0;
}
