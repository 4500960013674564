// order_guess_core.h -- the estimate behind FLACENC_HIP_FLAG_ORDER_GUESS (order_search.cpp's order_guess_kernel; DESIGN.md
// section 4.13), shared by the device kernel and a host build (tests/host/order_guess_core_test.cpp, compiled by g++):
// the prediction error the Levinson recursion leaves after every order, the bits per sample it stands for, the cost of
// coding the subframe at that order, and the K orders of the smallest (cost, order).  This is libFLAC's default order
// guess restated on this project's numbers; log2f comes in as a parameter (libm's on the host, dev_log2f on the device,
// the same function bit for bit).  Every translation unit that includes this is compiled with contraction off: the
// products and sums below are each rounded on their own.
#ifndef FLACENC_HIP_ORDER_GUESS_CORE_H_
#define FLACENC_HIP_ORDER_GUESS_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define OG_HD __host__ __device__ inline
#else
#define OG_HD inline
#endif

namespace order_guess {

constexpr uint32_t kMaxOrder = 32;

// e_o = e_(o-1) * (1.0 - k_o * k_o): multiply, subtract, multiply, no fma
OG_HD double error_step(double e_prev, double k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double kk = k * k;
  const double one_minus = 1.0 - kk;
  return e_prev * one_minus;
}

// b_o: the estimated bits per residual sample at prediction error e over a block of n samples; +0.0f where the estimate
// is not positive (x <= 0, a NaN, or log2 at or below zero)
template <typename Log2f>
OG_HD float bits_per_sample(double e, uint32_t n, Log2f log2f_fn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double scale = 0.5 / (double)n;
  const float x = (float)(e * scale);
  if (!(x > 0.0f)) return 0.0f;
  const float b = 0.5f * log2f_fn(x);
  return b > 0.0f ? b : 0.0f;
}

// cost_o = b_o (n - o) + o (q + w): the residual's estimated bits and the order's warm-up samples and coefficients
OG_HD double order_cost(float b, uint32_t n, uint32_t o, uint32_t q, uint32_t w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double resid = (double)b * (double)(n - o);
  return resid + (double)(o * (q + w));
}

struct Guess {
  uint32_t eligible;       // orders 1..eligible are eligible (the first failure ends the chain)
  uint32_t mask;           // bit o - 1: order o is a guess
  double cost[kMaxOrder];  // cost[o - 1] for o <= eligible
};

// One window's guesses.  r0 = R[0]; refl[(o - 1) * refl_stride] = k_o, the last unquantised coefficient of candidate o;
// status[(o - 1) * status_stride] = that candidate's status.  Order o is eligible iff every candidate i <= o has status
// 0 and e_i >= 0 (e_0 = R[0]; a NaN fails); the guesses are the K eligible orders of the smallest (cost, order).
template <typename Log2f>
OG_HD void guess_orders(double r0, const double* refl, uint32_t refl_stride, const int32_t* status,
                        uint32_t status_stride, uint32_t P, uint32_t n, uint32_t w, uint32_t q, uint32_t K,
                        Log2f log2f_fn, Guess* out) {
  out->eligible = 0;
  out->mask = 0;
  double e = r0;
  if (e >= 0.0) {
    for (uint32_t o = 1; o <= P && o <= kMaxOrder; ++o) {
      if (status[(o - 1) * status_stride] != 0) break;
      e = error_step(e, refl[(o - 1) * refl_stride]);
      if (!(e >= 0.0)) break;
      out->cost[o - 1] = order_cost(bits_per_sample(e, n, log2f_fn), n, o, q, w);
      out->eligible = o;
    }
  }
  for (uint32_t pick = 0; pick < K && pick < out->eligible; ++pick) {
    uint32_t best = 0;
    for (uint32_t o = 1; o <= out->eligible; ++o) {
      if ((out->mask >> (o - 1)) & 1u) continue;
      if (best == 0 || out->cost[o - 1] < out->cost[best - 1]) best = o;  // strict: the lower order keeps a tie
    }
    out->mask |= 1u << (best - 1);
  }
}

}  // namespace order_guess
#endif
