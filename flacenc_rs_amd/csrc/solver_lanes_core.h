#ifndef FLACENC_HIP_SOLVER_LANES_CORE_H_
#define FLACENC_HIP_SOLVER_LANES_CORE_H_
// solver_lanes_core.h -- the arithmetic of the fused 4096 kernel's lane-parallel quantise-and-certify step
// (levinson_phase_lanes, qlpc_wave_kernel_impl.h), one coefficient or one system at a time, for the device and for the
// host (tests/host/solver_lanes_test.cpp holds the assembled result equal to levinson_quantize_full's).
//
// Every function here is a piece of levinson_quantize_full / quant_certified (qlpc_kernel_impl.h) cut where the lanes
// part: the same floating-point operations on the same operands in the same order -- only WHO issues them changes
// (one lane per coefficient instead of one lane walking its system's coefficients).  The two f64 sums whose rounding
// order reaches the certificate's bound (|a|_1 and |forward|_1) stay sequential, on the lane that ran the recursion
// (lanes_cert_bound).  Include behind qlpc_kernel_impl.h (or the host test's slice of it): kCertSafety and
// kCertOwnRoundings come from there.
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FLACENC_LANES_HD __host__ __device__ __forceinline__
#else
#define FLACENC_LANES_HD inline
#endif

namespace flacenc_hip {
namespace {

// ceil_log2_pos (qlpc_kernel_impl.h) for either side: exact ceil(log2(m)) from the exponent / mantissa fields
FLACENC_LANES_HD int lanes_ceil_log2_pos(double m) {
  uint64_t b;
  __builtin_memcpy(&b, &m, 8);
  const int e = (int)((b >> 52) & 0x7FF);
  const uint64_t frac = b & 0xFFFFFFFFFFFFFull;
  if (e == 0) return -32752;
  return (e - 1023) + (frac != 0 ? 1 : 0);
}

// v - floor(v) for 0 <= v < 2^52: v_fract_f64 on the device, as quant_certified has it
FLACENC_LANES_HD double lanes_fract(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fract(v);
#else
  return v - floor(v);
#endif
}

// find_shift (lpc.rs:234-254) from max |a|; *e_out = ceil(log2(max |a|)), which the certificate's gaps use again
FLACENC_LANES_HD int lanes_find_shift(double amax, int precision, int* e_out) {
  int abs_log2 = lanes_ceil_log2_pos(amax);
  *e_out = abs_log2;
  if (abs_log2 < -32752) abs_log2 = -32752;
  const int shift = (precision - 1) - abs_log2;
  return shift < 0 ? 0 : (shift > 15 ? 15 : shift);
}

// quantize_parameter (lpc.rs:258-270) for one coefficient: round half away from zero, the i16 clamp, the precision clamp.
// (The f64 clamp stays: with the shift clamped at 0 -- max |a| above 2^(precision - 1), which a system that is not
// positive definite can produce at any size -- nothing bounds a * scalefac, and the conversion needs its operand in range.)
FLACENC_LANES_HD int32_t lanes_quantize_one(double a, double scalefac, int lo, int hi) {
  double s = round(a * scalefac);
  s = s < -32768.0 ? -32768.0 : (s > 32767.0 ? 32767.0 : s);
  const int q = (int)s;
  return q < lo ? lo : (q > hi ? hi : q);
}

// The certificate's first tier, the part that belongs to the system (quant_certified up to its loop): max |a| -+ |da|
// stays inside (2^(e-1), 2^e]; everything multiplied through by f0 = |forward[0]|
FLACENC_LANES_HD bool lanes_certify_system(double amax, int e, double num, double f0) {
  const double g_lo = amax - ldexp(1.0, e - 1), g_hi = ldexp(1.0, e) - amax;
  return (amax > 0.0) & (num < g_lo * f0) & (num < g_hi * f0);  // (no short circuit: three compares, no branch)
}

// ... and the part that belongs to one coefficient (one trip of quant_certified's loop): a * scalefac stays further
// from a rounding boundary k + 1/2 than the bound; nums = num * scalefac
FLACENC_LANES_HD bool lanes_certify_one(double a, double scalefac, double f0, double nums) {
  const double v = fabs(a) * scalefac;
  const double d = fabs(lanes_fract(v) - 0.5);
  return d * f0 > nums;
}

// num = |da| |f0| of quant_certified, from the two sequential sums, on the lane that holds a[] and forward[]
template <int MAXP>
FLACENC_LANES_HD double lanes_cert_bound(const double (&a)[MAXP], const double (&fwd)[MAXP], double r0, uint32_t max_abs_s,
                                         int n_sum) {
  double a1 = 0.0, f1 = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < MAXP; ++i) f1 += fabs(fwd[i]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < MAXP; ++i) a1 += fabs(a[i]);
  const double m = (double)max_abs_s;
  const double S = r0 + (0.5 * (double)MAXP) * (m * m);
  const double eps = ((double)(n_sum + kCertOwnRoundings) * 0x1p-53) * S;
  const double eps_a = eps * (1.0 + a1);
  return ((kCertSafety * 2.0) * (f1 * f1)) * eps_a;
}

}  // namespace
}  // namespace flacenc_hip
#endif
