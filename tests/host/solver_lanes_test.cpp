// solver_lanes_test.cpp -- the fused kernel's lane-parallel quantise-and-certify step against levinson_quantize_full, on
// the host.  The per-coefficient and per-system arithmetic is solver_lanes_core.h itself (what the kernel's
// levinson_phase_lanes calls); this file assembles it the way the kernel's lanes do -- the recursion and the two
// sequential sums on a "leader", one coefficient per "lane", max |a| by the lanes' butterfly, order and the certificate's
// verdict from "ballots" -- and holds qc[], order, shift, certified, tier2 and redo equal to levinson_quantize_full's,
// whose text is cut from qlpc_kernel_impl.h by tests/test_solver_lanes_host.py (solver_slice.inc).  A second copy of that
// text (solver_slice_injected.inc, namespace inj) has its ONE call of levinson_core_full replaced by inject_core, which
// hands out a[] / forward[] the test chose: the quantiser's and the certificate's corners are reached by construction,
// not by hunting for an R[] that happens to produce them.  Build with -ffp-contract=off (as the kernels are).
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

namespace flacenc_hip {
namespace {
#include "solver_slice.inc"
}
}  // namespace flacenc_hip
#include "solver_lanes_core.h"

// what inject_core hands out
static double g_a[16], g_fwd[16];
static bool g_skipped, g_nonpd;
template <int MAXP>
static void inject_core(const double (&)[MAXP + 1], double (&a)[MAXP], double (&fwd)[MAXP], bool* skipped, bool* nonpd) {
  for (int i = 0; i < MAXP; ++i) {
    a[i] = g_a[i];
    fwd[i] = g_fwd[i];
  }
  *skipped |= g_skipped;
  *nonpd |= g_nonpd;
}
namespace inj {
#include "solver_slice_injected.inc"
}

using namespace flacenc_hip;

static int failures = 0;
static long n_cases = 0, n_redo = 0, n_certified = 0, n_tier2 = 0, n_clamp_lo = 0, n_clamp_hi = 0, n_short = 0;

struct Result {
  int32_t qc[16];
  int order, shift;
  bool certified, tier2, redo;
};

// levinson_phase_lanes on the host: lane i of the system's group holds coefficient i
template <int MAXP>
static Result lanes(const double (&a)[MAXP], const double (&fwd)[MAXP], double r0, bool skipped, bool nonpd, int precision,
                    uint32_t max_abs_s, int n_sum, bool do_cert) {
  constexpr int G = MAXP <= 8 ? 8 : 16;
  Result r{};
  // leader
  const bool lead_redo = skipped || !shim_class(r0, 0x180);
  double num = 0.0, f0 = 0.0;
  if (do_cert) {
    num = lanes_cert_bound<MAXP>(a, fwd, r0, max_abs_s, n_sum);
    f0 = fabs(fwd[0]);
  }
  // lanes
  double av[G], mx[G];
  bool valid[G];
  for (int i = 0; i < G; ++i) {
    valid[i] = i < MAXP;
    av[i] = valid[i] ? a[i] : 0.0;
    mx[i] = fabs(av[i]);
  }
  bool redo = lead_redo;
  for (int i = 0; i < G; ++i) redo = redo || shim_class(av[i], 0x207);
  // the butterfly: xor 1, xor 2, mirror inside 8, mirror inside 16
  auto step = [&](auto partner) {
    double nx[G];
    for (int i = 0; i < G; ++i) nx[i] = fmax(mx[i], mx[partner(i)]);
    for (int i = 0; i < G; ++i) mx[i] = nx[i];
  };
  step([](int i) { return i ^ 1; });
  step([](int i) { return i ^ 2; });
  step([](int i) { return (i & ~7) | (7 - (i & 7)); });
  if (G == 16) step([](int i) { return 15 - i; });
  uint32_t nz = 0, bad = 0;
  int shift_seen = -1;
  for (int i = 0; i < G; ++i) {
    const double amax = mx[i];
    int e;
    const int shift = lanes_find_shift(amax, precision, &e);
    if (i == 0) shift_seen = shift;
    if (shift != shift_seen) {
      std::printf("lanes of one group disagree on the shift\n");
      ++failures;
    }
    const double scalefac = (double)(1 << shift);
    const int lo = -(1 << (precision - 1)), hi = (1 << (precision - 1)) - 1;
    const int q = lanes_quantize_one(av[i], scalefac, lo, hi);
    if (valid[i]) r.qc[i] = q;
    if (valid[i] && q != 0) nz |= 1u << i;
    if (do_cert) {
      bool ok = lanes_certify_system(amax, e, num, f0);
      ok = lanes_certify_one(av[i], scalefac, f0, num * scalefac) && ok;
      if (valid[i] && !ok) bad |= 1u << i;
    }
  }
  r.order = nz != 0u ? 32 - __builtin_clz(nz) : 1;
  r.shift = shift_seen;
  r.certified = true;
  r.tier2 = false;
  if (do_cert) {
    r.certified = !nonpd && bad == 0u;
    r.tier2 = !nonpd && bad != 0u;
  }
  r.redo = redo;
  return r;
}

template <int MAXP>
static void compare(const Result& got, bool redo, const int32_t* qc, int order, int shift, bool certified, bool tier2,
                    int precision, bool do_cert, const char* what) {
  ++n_cases;
  bool ok = got.redo == redo;
  if (ok && redo) {
    ++n_redo;  // (the kernel solves again through the generic code: nothing else of either side is used)
    return;
  }
  ok = ok && got.order == order && got.shift == shift && got.certified == certified && got.tier2 == tier2;
  for (int i = 0; i < MAXP; ++i) ok = ok && got.qc[i] == qc[i];
  if (!ok) {
    std::printf("MISMATCH %s MAXP %d precision %d do_cert %d: redo %d/%d order %d/%d shift %d/%d certified %d/%d tier2 %d/%d\n", what,
                MAXP, precision, (int)do_cert, (int)redo, (int)got.redo, order, got.order, shift, got.shift, (int)certified,
                (int)got.certified, (int)tier2, (int)got.tier2);
    ++failures;
    return;
  }
  if (do_cert) {
    n_certified += certified;
    n_tier2 += tier2;
  }
  const int lo = -(1 << (precision - 1)), hi = (1 << (precision - 1)) - 1;
  for (int i = 0; i < MAXP; ++i) {
    n_clamp_lo += qc[i] == lo;
    n_clamp_hi += qc[i] == hi;
  }
  n_short += order < MAXP;
}

// a system through the real recursion: levinson_quantize_full on R[] against the lanes on levinson_core_full's a[] / forward[]
template <int MAXP>
static void from_r(const double* Rl, uint32_t max_abs_s, const char* what) {
  for (int precision : {3, 8, 15})
    for (bool do_cert : {true, false}) {
      double af[MAXP];
      int32_t qf[MAXP];
      int of = -1, sf = -1;
      bool cf = true, tf = false;
      const bool redo = levinson_quantize_full<MAXP, true>(Rl, precision, af, qf, &of, &sf, max_abs_s, 4096, &cf, &tf, do_cert);
      double R[MAXP + 1], a[MAXP], fwd[MAXP];
      for (int i = 0; i <= MAXP; ++i) R[i] = Rl[i];
      bool skipped = false, nonpd = false;
      levinson_core_full<MAXP>(R, a, fwd, &skipped, &nonpd);
      const Result got = lanes<MAXP>(a, fwd, R[0], skipped, nonpd, precision, max_abs_s, 4096, do_cert);
      compare<MAXP>(got, redo, qf, of, sf, cf, tf, precision, do_cert, what);
    }
}

// chosen a[] / forward[]: the injected copy of levinson_quantize_full against the lanes on the same values
template <int MAXP>
static void from_a(const double* a_in, const double* fwd_in, double r0, uint32_t max_abs_s, bool skipped, bool nonpd,
                   int precision, const char* what) {
  double a[MAXP], fwd[MAXP], Rl[MAXP + 1];
  for (int i = 0; i < MAXP; ++i) {
    g_a[i] = a[i] = a_in[i];
    g_fwd[i] = fwd[i] = fwd_in[i];
  }
  for (int i = 0; i <= MAXP; ++i) Rl[i] = i == 0 ? r0 : 0.0;
  g_skipped = skipped;
  g_nonpd = nonpd;
  for (bool do_cert : {true, false}) {
    double af[MAXP];
    int32_t qf[MAXP];
    int of = -1, sf = -1;
    bool cf = true, tf = false;
    const bool redo = inj::levinson_quantize_full<MAXP, true>(Rl, precision, af, qf, &of, &sf, max_abs_s, 4096, &cf, &tf, do_cert);
    const Result got = lanes<MAXP>(a, fwd, r0, skipped, nonpd, precision, max_abs_s, 4096, do_cert);
    compare<MAXP>(got, redo, qf, of, sf, cf, tf, precision, do_cert, what);
  }
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

// the systems of solver_full_order_test.cpp (same generators, same seeds)
template <int MAXP>
static void suite_systems() {
  std::mt19937_64 rng(0xF1AC0000u + MAXP);
  std::normal_distribution<double> gauss(0.0, 1.0);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  double R[MAXP + 1];
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
    from_r<MAXP>(R, (uint32_t)m, "material");
  }
  for (int it = 0; it < 400; ++it) {
    std::vector<double> x(4096);
    const double w = it < 200 ? 3.14159265358979 * (it + 1) / 201.0 : 0.0;
    for (int t = 0; t < 4096; ++t) x[t] = it < 200 ? std::nearbyint(32767.0 * std::sin(w * t + 0.3)) : (it % 2 ? 12345.0 - it : ((t & 1) ? 32767.0 : -32768.0));
    acorr<MAXP>(x, R);
    from_r<MAXP>(R, 32768u, "near-singular");
  }
  for (int k = 0; k <= MAXP; ++k) R[k] = 0.0;
  from_r<MAXP>(R, 0u, "silence");
  R[0] = 1024.0;
  from_r<MAXP>(R, 32u, "impulse");
  for (double r1 : {1024.0, -1024.0}) {
    R[1] = r1;
    for (int k = 2; k <= MAXP; ++k) R[k] = (k & 1) ? r1 : 1024.0;
    from_r<MAXP>(R, 32u, "zero denominator");
  }
  for (int it = 0; it < 2000; ++it) {
    const double scale = std::ldexp(1.0, (int)(rng() % 120) - 20);
    for (int k = 0; k <= MAXP; ++k) R[k] = scale * uni(rng);
    R[0] = std::fabs(R[0]) * (it % 3 ? 1.0 : 4.0);
    if (it % 7 == 0) R[1 + rng() % MAXP] *= 1e300;
    if (it % 11 == 0) R[rng() % (MAXP + 1)] = it % 2 ? INFINITY : NAN;
    if (it % 13 == 0) R[0] = -R[0];
    if (it % 17 == 0) R[0] = 0.0;
    from_r<MAXP>(R, 32768u, "arbitrary");
  }
}

#define EXPECT(cond, what)                                              \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("EXPECT failed (MAXP %d) %s: %s\n", MAXP, what, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// the constructed corners
template <int MAXP>
static void suite_corners() {
  std::mt19937_64 rng(0x1A9E5000u + MAXP);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  double a[MAXP], fwd[MAXP];
  // a forward vector under which well-placed coefficients certify: |f|_1 close to |f_0|
  auto quiet_fwd = [&]() {
    for (int i = 0; i < MAXP; ++i) fwd[i] = i == 0 ? 1.0 / 1.0e9 : 1.0e-12 * uni(rng);
  };
  for (int precision : {3, 8, 15}) {
    const int lo = -(1 << (precision - 1)), hi = (1 << (precision - 1)) - 1;
    const double sc = (double)(1 << (precision - 1));  // the scale factor while 1/2 < max |a| <= 1
    quiet_fwd();
    // a * scalefac exactly at k + 0.5, both signs, every position (a[0] or a[1] = 0.75 pins the shift at precision - 1)
    for (int pos = 0; pos < MAXP; ++pos)
      for (int k = 0; k < hi - 1; k += (hi > 16 ? hi / 13 : 1))
        for (double sign : {1.0, -1.0}) {
          for (int i = 0; i < MAXP; ++i) a[i] = 0.0;
          a[pos == 0 ? 1 : 0] = 0.75;
          a[pos] = sign * ((double)k + 0.5) / sc;
          from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "half");
        }
    // clamps: +1.0 quantises to 2^(precision-1), above hi; -1.0 lands on lo; with the shift clamped at 0 anything goes
    for (int pos = 0; pos < MAXP; ++pos)
      for (double big : {1.0, -1.0, 1000.25, -1000.25, 40000.0, -40000.0, 1.0e6, -1.0e6, 3.0e9, -3.0e9, 1.0e300, -1.0e300}) {
        for (int i = 0; i < MAXP; ++i) a[i] = 0.1 * uni(rng);
        a[pos] = big;
        const long lo_before = n_clamp_lo, hi_before = n_clamp_hi;
        from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "clamp");
        // (1000.25 keeps a shift above 0 at precision 15 and stays inside: no claim there)
        if (std::fabs(big) == 1.0 || std::fabs(big) >= 40000.0)
          EXPECT(big > 0 ? n_clamp_hi > hi_before : n_clamp_lo > lo_before, "the big coefficient ends at the precision's bound");
      }
    // trailing coefficients that quantise to zero: order truncation down to 1
    for (int keep = 1; keep <= MAXP; ++keep) {
      for (int i = 0; i < MAXP; ++i) a[i] = i < keep ? (i & 1 ? -0.7 : 0.6) : 0.49 / sc * uni(rng);
      const long before = n_short;
      from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "truncation");
      if (keep < MAXP) EXPECT(n_short > before, "trailing zeros shorten the order");
    }
    // shift 0 (max |a| >= 2^(precision-1)) and shift 15 (tiny coefficients), all-zero a[]
    for (double scale : {(double)(1 << (precision - 1)), 3.0 * (1 << (precision - 1)), 1.0e-4, 1.0e-9, 1.0e-300, 0.0})
      for (int rep = 0; rep < 8; ++rep) {
        for (int i = 0; i < MAXP; ++i) a[i] = scale * uni(rng);
        a[rep % MAXP] = (rep & 1) ? -scale : scale;
        from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "shift edge");
      }
    // max |a| an exact power of two: the upper find_shift gap is zero
    for (int ex = -24; ex <= 6; ++ex)
      for (int pos = 0; pos < MAXP; ++pos) {
        for (int i = 0; i < MAXP; ++i) a[i] = std::ldexp(0.3 * uni(rng), ex);
        a[pos] = std::ldexp((pos & 1) ? -1.0 : 1.0, ex);
        const long before = n_certified;
        from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "power of two");
        EXPECT(n_certified == before, "no certificate at a power of two");
      }
    // a NaN and an infinity in each position; the leader's own reasons for the second solve
    for (int pos = 0; pos < MAXP; ++pos)
      for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
        for (int i = 0; i < MAXP; ++i) a[i] = 0.4 * uni(rng);
        a[pos] = bad;
        const long before = n_redo;
        from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, false, precision, "non-finite");
        EXPECT(n_redo == before + 2, "a non-finite coefficient asks for the second solve");
      }
    for (int i = 0; i < MAXP; ++i) a[i] = 0.4 * uni(rng);
    from_a<MAXP>(a, fwd, 1.0e9, 1000u, true, false, precision, "skipped");
    from_a<MAXP>(a, fwd, 0.0, 1000u, false, false, precision, "r0 zero");
    from_a<MAXP>(a, fwd, -1.0, 1000u, false, false, precision, "r0 negative");
    from_a<MAXP>(a, fwd, 1.0e9, 1000u, false, true, precision, "nonpd");
    // random coefficients under forward vectors and energies that put the bound on either side of the gaps
    for (int it = 0; it < 4000; ++it) {
      const double scale = std::ldexp(1.0, (int)(rng() % 12) - 8);
      for (int i = 0; i < MAXP; ++i) a[i] = scale * uni(rng);
      const double r0 = std::ldexp(1.0 + std::fabs(uni(rng)), 10 + (int)(rng() % 40));
      const double spread = std::ldexp(1.0, -(int)(rng() % 40));
      for (int i = 0; i < MAXP; ++i) fwd[i] = (i == 0 ? 1.0 : spread * uni(rng)) / r0;
      from_a<MAXP>(a, fwd, r0, (uint32_t)(rng() % 32769), false, it % 50 == 0, precision, "random");
    }
  }
}

int main() {
  suite_systems<8>();
  suite_systems<10>();
  suite_systems<12>();
  const long systems = n_cases;
  suite_corners<8>();
  suite_corners<10>();
  suite_corners<12>();
  std::printf("%ld cases (%ld through the recursion), %ld asked for the second solve, %ld certified, %ld second tier, "
              "%ld at lo, %ld at hi, %ld shortened, %d failures\n",
              n_cases, systems, n_redo, n_certified, n_tier2, n_clamp_lo, n_clamp_hi, n_short, failures);
  return failures ? 1 : 0;
}
