// solver_full_order_test.cpp -- the straight-line full-order solver of the fused kernel (levinson_quantize_full,
// qlpc_kernel_impl.h) against the generic one (levinson_quantize at P == MAXP), compiled for the host from the very text
// of the header (solver_slice.inc: cut out by tests/test_solver_full_order_host.py) behind a few shims for the device
// builtins.  Contract: whenever levinson_quantize_full does not ask for the second solve (`redo`), the generic code's
// status is 0 and every output -- coefficients bit for bit, quantised coefficients, order, shift, the certificate's two
// flags -- is the generic code's; and it asks for the second solve only where the generic code leaves the straight line
// (a zero denominator, R[0] not above zero, a status).  Build with -ffp-contract=off (as the kernels are).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define FLACENC_HIP_SUBFRAME_OK 0
#define FLACENC_HIP_SUBFRAME_NONFINITE 1
#define FLACENC_HIP_SUBFRAME_NEG_ENERGY 2
#define __device__
#define __forceinline__ inline
static inline long long __double_as_longlong(double d) { long long v; std::memcpy(&v, &d, 8); return v; }
static inline double shim_fract(double v) { return v - std::floor(v); }          // (v_fract_f64 for 0 <= v < 2^52)
static inline bool shim_class(double v, int mask) {  // v_cmp_class_f64: the two masks the solver uses
  if (mask == 0x207) return !std::isfinite(v);              // NaN, -inf, +inf
  if (mask == 0x180) return std::isfinite(v) && v > 0.0;    // +subnormal, +normal
  std::abort();
}
#define __builtin_amdgcn_fract shim_fract
#define __builtin_amdgcn_class shim_class
using std::ceil; using std::fabs; using std::floor; using std::fmax; using std::ldexp; using std::round;

#include "solver_slice.inc"

static int failures = 0;
static long n_cases = 0, n_redo = 0;

static bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

template <int MAXP, bool CERT>
static bool one(const double* R, int precision, uint32_t max_abs_s, bool do_cert, const char* what) {
  double ag[MAXP], af[MAXP];
  int32_t qg[MAXP], qf[MAXP];
  int og = -1, sg = -1, of = -1, sf = -1;
  bool cg = true, tg = false, cf = true, tf = false;
  int st;
  if (CERT)
    st = levinson_quantize<MAXP, true>(R, MAXP, precision, ag, qg, &og, &sg, max_abs_s, 4096, &cg, &tg, do_cert);
  else
    st = levinson_quantize<MAXP>(R, MAXP, precision, ag, qg, &og, &sg);
  const bool redo = levinson_quantize_full<MAXP, CERT>(R, precision, af, qf, &of, &sf, max_abs_s, 4096, &cf, &tf, do_cert);
  ++n_cases;
  if (redo) {
    ++n_redo;
    return true;
  }
  bool ok = st == 0 && og == of && sg == sf && cg == cf && tg == tf;
  for (int i = 0; i < MAXP; ++i) ok = ok && same_bits(ag[i], af[i]) && qg[i] == qf[i];
  if (!ok) {
    std::printf("MISMATCH %s MAXP %d CERT %d precision %d do_cert %d: status %d order %d/%d shift %d/%d certified %d/%d tier2 %d/%d\n",
                what, MAXP, (int)CERT, precision, (int)do_cert, st, og, of, sg, sf, (int)cg, (int)cf, (int)tg, (int)tf);
    ++failures;
  }
  return false;
}

template <int MAXP>
static bool all_forms(const double* R, uint32_t max_abs_s, const char* what) {
  bool redo = false;
  for (int precision : {3, 8, 15}) {
    redo |= one<MAXP, true>(R, precision, max_abs_s, true, what);
    redo |= one<MAXP, true>(R, precision, max_abs_s, false, what);
    redo |= one<MAXP, false>(R, precision, max_abs_s, false, what);
  }
  return redo;
}

// R[k] = sum_{t >= MAXP} x[t] x[t - k], as the kernels sum it (any order: only the solver is under test)
template <int MAXP>
static void acorr(const std::vector<double>& x, double* R) {
  for (int k = 0; k <= MAXP; ++k) {
    double s = 0.0;
    for (size_t t = MAXP; t < x.size(); ++t) s = std::fma(x[t], x[t - k], s);
    R[k] = s;
  }
}

#define EXPECT(cond, what)                                              \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("EXPECT failed (MAXP %d) %s: %s\n", MAXP, what, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

template <int MAXP>
static void suite() {
  std::mt19937_64 rng(0xF1AC0000u + MAXP);
  std::normal_distribution<double> gauss(0.0, 1.0);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  double R[MAXP + 1];
  // material: noise, AR processes (never a second solve), tones in noise
  for (int it = 0; it < 3000; ++it) {
    const int n = 4096;
    std::vector<double> x(n);
    const int kind = it % 4;
    const double c1 = uni(rng) * 1.8, c2 = -0.95 * std::fabs(uni(rng)), w = 0.01 + 3.0 * std::fabs(uni(rng));
    double m = 0.0;
    for (int t = 0; t < n; ++t) {
      double v = 3000.0 * gauss(rng);
      if (kind == 1 && t >= 2) v = 300.0 * gauss(rng) + c1 * x[t - 1] + (std::fabs(c1) < 1.0 ? 0.0 : c2 * x[t - 2]);
      if (kind == 2) v = 20000.0 * std::sin(w * t) + 30.0 * gauss(rng);
      if (kind == 3) v = 12000.0 * std::sin(w * t) + 9000.0 * std::sin(0.37 * w * t + 1.0) + gauss(rng);
      v = std::nearbyint(std::fmax(-32768.0, std::fmin(32767.0, v)));
      x[t] = v;
      m = std::fmax(m, std::fabs(v));
    }
    acorr<MAXP>(x, R);
    const bool redo = all_forms<MAXP>(R, (uint32_t)m, "material");
    // (tones with a trace of noise can round a denominator to exactly zero at the higher steps: the generic code skips there)
    if (kind == 0 || (kind == 1 && std::fabs(c1) < 1.0)) EXPECT(!redo, "well-conditioned material stays on the straight line");
  }
  // pure tones, constants, alternation: near-singular systems (the outputs must still agree wherever no second solve is asked)
  for (int it = 0; it < 400; ++it) {
    std::vector<double> x(4096);
    const double w = it < 200 ? 3.14159265358979 * (it + 1) / 201.0 : 0.0;
    for (int t = 0; t < 4096; ++t) x[t] = it < 200 ? std::nearbyint(32767.0 * std::sin(w * t + 0.3)) : (it % 2 ? 12345.0 - it : ((t & 1) ? 32767.0 : -32768.0));
    acorr<MAXP>(x, R);
    all_forms<MAXP>(R, 32768u, "near-singular");
  }
  // the corners the generic code branches on
  for (int k = 0; k <= MAXP; ++k) R[k] = 0.0;
  EXPECT(all_forms<MAXP>(R, 0u, "silence"), "digital silence takes the second solve");
  R[0] = 1024.0;  // an impulse: every coefficient is zero, no second solve
  EXPECT(!all_forms<MAXP>(R, 32u, "impulse"), "R = (r0, 0, ...) stays on the straight line");
  for (double r1 : {1024.0, -1024.0}) {  // err = +-1 exactly: the denominator of step 1 is zero, the generic code skips the step
    R[1] = r1;
    for (int k = 2; k <= MAXP; ++k) R[k] = (k & 1) ? r1 : 1024.0;
    EXPECT(all_forms<MAXP>(R, 32u, "zero denominator"), "a zero denominator takes the second solve");
  }
  for (int it = 0; it < 2000; ++it) {  // arbitrary R[]: not autocorrelations, negative denominators, overflow, non-finite entries
    const double scale = std::ldexp(1.0, (int)(rng() % 120) - 20);
    for (int k = 0; k <= MAXP; ++k) R[k] = scale * uni(rng);
    R[0] = std::fabs(R[0]) * (it % 3 ? 1.0 : 4.0);
    if (it % 7 == 0) R[1 + rng() % MAXP] *= 1e300;
    if (it % 11 == 0) R[rng() % (MAXP + 1)] = it % 2 ? INFINITY : NAN;
    if (it % 13 == 0) R[0] = -R[0];
    if (it % 17 == 0) R[0] = 0.0;
    const bool redo = all_forms<MAXP>(R, 32768u, "arbitrary");
    if (!(R[0] > 0.0)) EXPECT(redo, "R[0] not above zero takes the second solve");
    bool finite = true;
    for (int k = 0; k <= MAXP; ++k) finite = finite && std::isfinite(R[k]);
    if (!finite) EXPECT(redo, "a non-finite R[] takes the second solve");
  }
}

int main() {
  suite<8>();
  suite<10>();
  suite<12>();
  std::printf("%ld cases, %ld asked for the second solve, %d failures\n", n_cases, n_redo, failures);
  return failures ? 1 : 0;
}
