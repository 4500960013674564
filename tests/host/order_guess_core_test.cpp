// order_guess_core_test.cpp -- flacenc_rs_amd/csrc/order_guess_core.h compiled for the host (g++, contraction off, also
// under ASan + UBSan; tests/test_order_guess_cpu.py), log2f from libm.  Reads cases from a file, writes the core's answers:
//   in : u32 count, then per case u32 P, n, w, q, K; f64 R[0]; f64 k[32]; i32 status[32]
//   out: per case u32 eligible, u32 mask, f64 cost[32] (zeros from `eligible` on)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "order_guess_core.h"

struct CaseIn {
  uint32_t P, n, w, q, K;
  uint32_t pad;
  double r0;
  double k[32];
  int32_t status[32];
};
struct CaseOut {
  uint32_t eligible, mask;
  double cost[32];
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, in) != 1) return 2;
  uint32_t pad = 0;
  if (fread(&pad, 4, 1, in) != 1) return 2;
  std::vector<CaseIn> cases(count);
  if (count && fread(cases.data(), sizeof(CaseIn), count, in) != count) return 2;
  fclose(in);
  std::vector<CaseOut> outs(count);
  for (uint32_t i = 0; i < count; ++i) {
    const CaseIn& c = cases[i];
    // exact-size copies: a read past order P shows under the sanitizer
    std::vector<double> k(c.k, c.k + c.P);
    std::vector<int32_t> st(c.status, c.status + c.P);
    order_guess::Guess g;
    order_guess::guess_orders(c.r0, k.data(), 1u, st.data(), 1u, c.P, c.n, c.w, c.q, c.K,
                              [](float x) { return log2f(x); }, &g);
    memset(&outs[i], 0, sizeof(CaseOut));
    outs[i].eligible = g.eligible;
    outs[i].mask = g.mask;
    for (uint32_t o = 0; o < g.eligible; ++o) outs[i].cost[o] = g.cost[o];
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  if (count && fwrite(outs.data(), sizeof(CaseOut), count, out) != count) return 2;
  fclose(out);
  printf("%u cases\n", count);
  return 0;
}
