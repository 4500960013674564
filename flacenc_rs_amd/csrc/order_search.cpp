// order_search.cpp -- FLACENC_HIP_FLAG_ORDER_SEARCH and FLACENC_HIP_FLAG_WINDOW_SEARCH (DESIGN.md sections 4.10, 4.11):
// per QLPC candidate subframe, the candidate (window j, order o) whose exact Lpc::count_bits is smallest.  Every candidate
// of window j comes from the one R_j[0..P] the reference-order pass produces under that window: levinson_quantize at order
// o reads lags 0..o only, so candidate (j, o) is bit for bit the order-o run under window j, and candidate (0, P) is the
// unflagged FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER record.  ORDER_SEARCH alone is the W = 1 case.
// FLACENC_HIP_FLAG_ORDER_GUESS (section 4.13) runs the same grid of predictors, then order_guess_kernel strikes every
// candidate that is neither (0, P) nor one of its window's K guesses (order_guess_core.h) before the search codes the rest.
// FLACENC_HIP_FLAG_PRECISION_SEARCH (section 4.16) is the third axis: every (j, o) is quantised at the Q precisions
// q0, q0 - 1, .. q0 - Q + 1 from the one run of the recursion, and the key takes each record's own precision.
#include "order_search.h"

#include "acorr_reference.h"
#include "lds_opt_in.h"
#include "order_guess_core.h"
#include "qlpc_kernel_impl.h"

namespace flacenc_hip {
namespace {

constexpr int kOsThreads = 256;
constexpr int kTabStride = 31;                    // Rice parameters 0..30 per partition row
constexpr uint32_t kMaxBits = (1u << 27) - 1u;    // MAX_P_TO_BITS, rice.rs:51
constexpr uint32_t kWideU = 1u << 27;             // zig-zag codes from here on can wrap a 16-sample chunk's u32 sum
constexpr size_t kCandWords = 36;                 // qc[32], order, shift, status, precision (levinson_batch_kernel's
                                                  // record, whose last word is 0: the launch's precision)
constexpr int32_t kNotCandidate = 0x40000000;     // order_guess_kernel's status word of a candidate the search skips
static_assert(sizeof(order_guess::Guess) == 264, "the trace record of flacenc_hip_debug_set_order_guess_trace");
constexpr size_t kSmallBytes = 1024 + 16 * 8 + 2 * 8 + 16 * 4 + 256 + 256;  // psum, level bits, sums, misc, two ps rows

enum { kMaxAbs = 0, kUMax, kSat, kLo, kHi, kRice2, kClamp };

struct OrderSearchArgs {
  const int32_t* samples;
  size_t stride;
  uint32_t block_size;
  uint32_t n_subframes;
  uint32_t stereo;
  const uint8_t* bps;
  uint32_t bps_uniform;
  uint32_t lpc_order;
  uint32_t n_cand;      // C candidates per subframe
  uint32_t max_rice_parameter;
  uint32_t rice_finest_only;
  const int32_t* cand;  // [n][C][36]
  uint32_t* best;       // [n]: chosen candidate + 1, 0 = no candidate with status 0
  int32_t* residual;    // zig-zag rows of the order under test when they do not fit the LDS (the output rows; stage 3
  size_t residual_stride;  // overwrites them)
};

__host__ __device__ inline int finest_order(int n) {  // finest_partition_order(n, 64), rice.rs:157-165 (warm-up <= 32)
  const unsigned max_splits = (unsigned)n / 64u;
  int lg = 0;
  while ((2u << lg) <= max_splits) ++lg;
  int tz = 0;
  while (((n >> tz) & 1) == 0 && tz < 15) ++tz;
  const int fo = lg < tz ? lg : tz;
  return fo < 8 ? fo : 8;
}

__host__ __device__ inline size_t round16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

size_t search_lds_bytes(uint32_t n, bool lds_u) {
  const size_t parts = static_cast<size_t>(1) << finest_order(static_cast<int>(n));
  return round16(4 * static_cast<size_t>(n)) * (lds_u ? 2 : 1) + round16(parts * kTabStride * 4) + kSmallBytes;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Candidate c = (j * Pc + (o - 1 - (P - Pc))) * Q + i of a subframe: window j, order o (Pc = P orders per window with the
// order search, else 1: order P only), precision q0 - i (Q = 1 without the precision search).  R_j of subframe sf at
// racc[(sf * W + j) * 33].
__device__ __forceinline__ void candidate_of(uint32_t c, uint32_t P, uint32_t Pc, uint32_t Q, uint32_t* j, int* o,
                                             uint32_t* i) {
  const uint32_t g = c / Q;
  *i = c % Q;
  *j = g / Pc;
  *o = (int)(P - Pc + 1u + g % Pc);
}

// quantize_parameters (lpc.rs:273-302: find_shift :234-254, quantize_parameter :258-270, the tail-zero truncation) of the
// coefficients a[0..P) of a levinson_quantize run with status 0, at another precision: operation for operation
// levinson_quantize's own quantiser, which stays as it is (the fused kernel's schedule hangs on that function's shape).
template <int MAXP>
__device__ void quantize_at(const double (&a)[MAXP], int P, int precision, int32_t* qc_out, int* order_out,
                            int* shift_out) {
  double max_abs = 0.0;
#pragma unroll
  for (int i = 0; i < MAXP; ++i)
    if (i < P) max_abs = fmax(max_abs, fabs(a[i]));
  int abs_log2 = ceil_log2_pos(max_abs);
  if (abs_log2 < -32752) abs_log2 = -32752;
  int shift = (precision - 1) - abs_log2;
  shift = shift < 0 ? 0 : (shift > 15 ? 15 : shift);
  const double scalefac = (double)(1 << shift);
  const int lo = -(1 << (precision - 1)), hi = (1 << (precision - 1)) - 1;
  int order = 1;
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    int q = 0;
    if (i < P) {
      double s = round(a[i] * scalefac);  // half away from zero
      s = s < -32768.0 ? -32768.0 : (s > 32767.0 ? 32767.0 : s);
      q = (int)s;
      q = q < lo ? lo : (q > hi ? hi : q);
      if (q != 0) order = i + 1;  // tail-zero truncation, min 1 (lpc.rs:295-299)
    }
    qc_out[i] = q;
  }
  *order_out = order;
  *shift_out = shift;
}

// a predictor record: qc[32], order, shift, status, precision
template <int MAXP>
__device__ __forceinline__ void write_pred(int32_t* pr, const int32_t* qc, int order, int shift, int status,
                                           uint32_t precision) {
#pragma unroll
  for (int k = 0; k < MAXP; ++k) pr[k] = qc[k];
  for (int k = MAXP; k < 32; ++k) pr[k] = 0;
  pr[32] = order;
  pr[33] = shift;
  pr[34] = status;
  pr[35] = (int32_t)precision;
}

// One lane per (subframe, window, order): the Q candidates (j, o, 0..Q-1) of subframe sf from [(sf * C + c) * 36] on:
// levinson_quantize on R_j[0..o] (lpc.rs:633-705, 273-302) at q0, then the same coefficients quantised at q0 - 1, ..
// (a status other than 0 is every precision's)
// REFL (the order guess): k_o, the candidate's unquantised coefficient number o - 1, at refl[sf * W * Pc + j * Pc + oi] as well
template <int MAXP, bool REFL>
__global__ void __launch_bounds__(64) order_levinson_kernel(const double* __restrict__ racc, uint32_t n_subframes,
                                                             uint32_t W, uint32_t P, uint32_t Pc, uint32_t Q,
                                                             uint32_t precision, int32_t* __restrict__ cand,
                                                             double* __restrict__ refl) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  const uint32_t G = W * Pc;
  if (i >= (size_t)n_subframes * G) return;
  const size_t sf = i / G;
  uint32_t j, i0;
  int o;
  candidate_of((uint32_t)(i % G) * Q, P, Pc, Q, &j, &o, &i0);
  double coef[MAXP];
  int32_t qc[MAXP];
  int order, shift;
  const int status = levinson_quantize<MAXP>(racc + (sf * W + j) * 33, o, (int)precision, coef, qc, &order, &shift);
  int32_t* pr = cand + i * Q * kCandWords;
  write_pred<MAXP>(pr, qc, order, shift, status, precision);
  for (uint32_t x = 1; x < Q; ++x) {
    if (status == 0) quantize_at<MAXP>(coef, o, (int)(precision - x), qc, &order, &shift);
    write_pred<MAXP>(pr + x * kCandWords, qc, order, shift, status, precision - x);
  }
  if (REFL) {
    double k = 0.0;
#pragma unroll
    for (int t = 0; t < MAXP; ++t) k = (t == o - 1) ? coef[t] : k;
    refl[i] = k;
  }
}

struct DevLog2f {
  __device__ float operator()(float x) const { return dev_log2f(x); }
};

// The order guess, one lane per (subframe, window): the error chain over the window's P candidates, the K guesses
// (order_guess_core.h), and kNotCandidate into the status word of every candidate that is neither a guess nor (0, P) --
// order_search_kernel skips a record whose status is not 0, and order_pick_kernel runs the chosen (j, o) again.
__global__ void __launch_bounds__(64) order_guess_kernel(const double* __restrict__ racc, const double* __restrict__ refl,
                                                          int32_t* __restrict__ cand, uint32_t n_subframes, uint32_t W,
                                                          uint32_t P, uint32_t Q, uint32_t precision, uint32_t block_size,
                                                          const uint8_t* __restrict__ bps, uint32_t bps_uniform,
                                                          uint32_t stereo, uint32_t K,
                                                          order_guess::Guess* __restrict__ trace) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  if (i >= (size_t)n_subframes * W) return;
  const size_t sf = i / W;
  const uint32_t j = (uint32_t)(i % W);
  const uint32_t w = bps ? (uint32_t)bps[sf] : bps_uniform + ((stereo && (sf & 3u) == 3u) ? 1u : 0u);
  const size_t c0 = i * P;  // (j, 1) of the subframe: sf * W * P + j * P; its Q records from c0 * Q on
  int32_t* st = cand + c0 * Q * kCandWords + 34;  // the status words of the records at q0, Q records apart
  order_guess::Guess g;
  order_guess::guess_orders(racc[i * 33], refl + c0, 1u, st, (uint32_t)(Q * kCandWords), P, block_size, w, precision, K,
                            DevLog2f(), &g);
  for (uint32_t o = 1; o <= P; ++o) {
    const bool keep = ((g.mask >> (o - 1)) & 1u) != 0u || (j == 0u && o == P);
    if (!keep)
      for (uint32_t x = 0; x < Q; ++x) st[((size_t)(o - 1) * Q + x) * kCandWords] = kNotCandidate;
  }
  if (trace) {  // test hook (flacenc_hip_debug.h): the lane's record, +0.0 above `eligible`; `trace` is lane 0's
    order_guess::Guess* t = trace + i;
    t->eligible = g.eligible;
    t->mask = g.mask;
    for (uint32_t o = 0; o < order_guess::kMaxOrder; ++o) t->cost[o] = o < g.eligible ? g.cost[o] : 0.0;
  }
}

// the chosen candidate's predictor record for the stage-3 kernels (its precision in word 35 with the precision search,
// else 0: the launch's), its unquantised coefficients (zeros from o on) and its window's R[0..P] (zeros above P)
template <int MAXP>
__global__ void __launch_bounds__(64) order_pick_kernel(const double* __restrict__ racc, uint32_t n_subframes, uint32_t W,
                                                         uint32_t P, uint32_t Pc, uint32_t Q, uint32_t precision,
                                                         const uint32_t* __restrict__ best, int32_t* __restrict__ pred,
                                                         double* __restrict__ lpc_coefs, double* __restrict__ autocorr) {
  const size_t sf = (size_t)blockIdx.x * 64u + threadIdx.x;
  if (sf >= n_subframes) return;
  const uint32_t b = best[sf];
  // no candidate with status 0: candidate (0, P, q0), status included
  const uint32_t c = (b >= 1u && b <= W * Pc * Q) ? b - 1u : (Pc - 1u) * Q;
  uint32_t j, x;
  int o;
  candidate_of(c, P, Pc, Q, &j, &o, &x);
  const double* rj = racc + (sf * W + j) * 33;
  double coef[MAXP];
  int32_t qc[MAXP];
  int order, shift;
  const int status = levinson_quantize<MAXP>(rj, o, (int)precision, coef, qc, &order, &shift);
  if (x != 0u && status == 0) quantize_at<MAXP>(coef, o, (int)(precision - x), qc, &order, &shift);
  write_pred<MAXP>(pred + sf * kCandWords, qc, order, shift, status, Q > 1u ? precision - x : 0u);
  if (lpc_coefs) {
#pragma unroll
    for (int k = 0; k < MAXP; ++k) lpc_coefs[sf * 32 + k] = (k < o && status == 0) ? coef[k] : 0.0;
    for (int k = MAXP; k < 32; ++k) lpc_coefs[sf * 32 + k] = 0.0;
  }
  if (autocorr) {
    for (int k = 0; k < 33; ++k) autocorr[sf * 33 + k] = k <= (int)P ? rj[k] : 0.0;
  }
}

// One workgroup per subframe: the samples staged in LDS once, then for every candidate (j, o) with status 0 the residual
// (compute_error, lpc.rs:359-390), the finest partitions' Rice bit tables over a parameter window and the reference's
// merge / minimiser walk (PrcParameterFinder::find, rice.rs:246-298) -> the exact Lpc::count_bits (bitrepr.rs:492-499,
// 533-544) as the candidate's key.  LDS_U: the zig-zag residual row of the order under test lives in LDS (blocks up to
// 8192 samples), otherwise in the subframe's output row.
//
// The window: a table entry f(p) = sum(u >> p) + len (p + 1) + 4 has f(p + 1) - f(p) = len - sum(ceil((u >> p) / 2)), which
// does not decrease with p, and is > 0 once len 2^p > sum(u), < 0 while 3 len 2^p <= sum(u).  So every partition's minimisers
// lie in [lo_i, hi_i] (the smallest p with 3 len 2^p > S_i, resp. len 2^p > S_i, both capped at max_p), a merged table is
// a sum of such functions, and its minimisers lie inside [min lo_i, max hi_i]: outside it every table is strictly
// monotone.  The argument needs every entry to be min(MAX, exact sum): zig-zag codes below 2^27 (no 16-sample chunk can
// wrap the u32 accumulator) and every S_i below 2^32 here; otherwise the window is all of 0..max_p.  The entries
// themselves are always computed as the reference does -- u32 adds, the clamp after each 16-sample chunk.
//
// Saturated entries: when max_p caps hi_i far below the residual's scale, a merged partition's entries can all be
// MAX_P_TO_BITS, inside the window and (the table only grows away from it) outside.  The reference's minimiser then picks
// p = 0, and its count_bits is the true sum at p = 0, not the clamped table value.  So such a partition takes p = 0 here
// too, and a chosen level with one -- or any chosen level when codes reach 2^27 -- gets its key from a pass over the true
// quotients.  Otherwise (S_i of 2^32 and more included) every chosen entry is below MAX and hence the exact sum.
template <bool LDS_U>
__global__ void __launch_bounds__(kOsThreads) order_search_kernel(OrderSearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const uint32_t sf = blockIdx.x;
  const int n = (int)a.block_size;
  const int fo = finest_order(n);
  const int nparts = 1 << fo;
  const int psize = n >> fo;
  const uint32_t maxp = a.max_rice_parameter;

  unsigned char* p = smem;
  int32_t* sbuf = reinterpret_cast<int32_t*>(p);
  p += round16(4 * (size_t)n);
  uint32_t* ubuf;
  if (LDS_U) {
    ubuf = reinterpret_cast<uint32_t*>(p);
    p += round16(4 * (size_t)n);
  } else {
    ubuf = reinterpret_cast<uint32_t*>(a.residual + (size_t)sf * a.residual_stride);
  }
  uint32_t* tab = reinterpret_cast<uint32_t*>(p);
  p += round16((size_t)nparts * kTabStride * 4);
  uint32_t* psum = reinterpret_cast<uint32_t*>(p);
  p += 1024;
  unsigned long long* lvl_bits = reinterpret_cast<unsigned long long*>(p);
  p += 16 * 8;
  unsigned long long* acc64 = reinterpret_cast<unsigned long long*>(p);
  p += 2 * 8;
  uint32_t* misc = reinterpret_cast<uint32_t*>(p);
  p += 16 * 4;
  uint8_t* pl = p;
  p += 256;
  uint8_t* psel = p;

  // ---- load (stereo: roles L, R, M = (l + r) >> 1, S = l - r of frame sf / 4, coding.rs:476-484) ----
  const int role = a.stereo ? (int)(sf & 3u) : 0;
  const int32_t* src = a.stereo ? a.samples + (size_t)(2u * (sf >> 2) + (role == 1 ? 1u : 0u)) * a.stride
                                : a.samples + (size_t)sf * a.stride;
  const int32_t* src2 = src + a.stride;
  if (tid < 16) misc[tid] = 0u;
  __syncthreads();
  uint32_t my_max = 0;
  for (int t = tid; t < n; t += kOsThreads) {
    int32_t v = src[t];
    if (role == 2) v = (v + src2[t]) >> 1;
    else if (role == 3) v -= src2[t];
    sbuf[t] = v;
    const uint32_t av = (uint32_t)(v < 0 ? -(int64_t)v : (int64_t)v);
    my_max = my_max > av ? my_max : av;
  }
  my_max = wave_max_u32(my_max);
  if (lane == 0) atomicMax(&misc[kMaxAbs], my_max);
  __syncthreads();
  const uint64_t maxabs = misc[kMaxAbs];
  const unsigned long long bps = a.bps ? (unsigned long long)a.bps[sf]
                                       : (unsigned long long)(a.bps_uniform + (role == 3 ? 1u : 0u));

  unsigned long long best_key = ~0ull;
  uint32_t best_c = 0;
  const int C = (int)a.n_cand;
  for (int cand = 0; cand < C; ++cand) {
    const int32_t* pr = a.cand + ((size_t)sf * (size_t)C + (size_t)cand) * kCandWords;
    if (pr[34] != 0) continue;  // (uniform: every thread reads the same record)
    const int q = pr[32];
    const int shift = pr[33];
    const unsigned long long prec = (unsigned long long)(uint32_t)pr[35];  // (order_levinson_kernel: never 0)
    int32_t c[32];
    int64_t sumabs = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      c[j] = pr[j];
      sumabs += c[j] < 0 ? -(int64_t)c[j] : (int64_t)c[j];
    }
    // compute_error's i32 criterion (lpc.rs:361-377), and 24-bit operands for v_mad_i32_i24
    const bool narrow = maxabs * (uint64_t)sumabs < 0x7FFFFFFFull && maxabs < (1u << 23);

    __syncthreads();  // (the previous candidate's readers are done)
    if (tid < nparts) psum[tid] = 0u;
    if (tid < 16) lvl_bits[tid] = 0ull;
    if (tid < 2) acc64[tid] = 0ull;
    if (tid == 0) {
      misc[kUMax] = 0u;
      misc[kSat] = 0u;
      misc[kLo] = 31u;
      misc[kHi] = 0u;
      misc[kRice2] = 0u;
      misc[kClamp] = 0u;
    }
    __syncthreads();

    // ---- residual, zig-zag codes, per-partition sums of u ----
    uint32_t my_umax = 0;
    for (int base = 0; base < n; base += kOsThreads) {
      const int t = base + tid;
      uint32_t u = 0;
      if (t < n && t >= q) {
        const int32_t* h = sbuf + (t - 1);
        int32_t e;
        if (narrow) {
          int32_t acc = 0;
#pragma unroll
          for (int j = 0; j < 32; ++j)
            if (j < q) acc += __mul24(c[j], h[-j]);
          e = (int32_t)((uint32_t)sbuf[t] - (uint32_t)(acc >> shift));
        } else {
          int64_t acc = 0;
#pragma unroll
          for (int j = 0; j < 32; ++j)
            if (j < q) acc += (int64_t)c[j] * (int64_t)h[-j];
          e = (int32_t)(uint32_t)(uint64_t)((int64_t)sbuf[t] - (acc >> shift));
        }
        u = zigzag(e);
      }
      if (t < n) ubuf[t] = u;
      my_umax = my_umax > u ? my_umax : u;
      // a wave's 64 samples lie in at most two partitions (psize >= 64)
      const int w0 = base + 64 * wave;
      if (w0 < n) {
        const int pa = w0 / psize;
        const int mine = t < n ? t / psize : pa;
        const unsigned long long sa = wave_sum_u64(mine == pa ? (unsigned long long)u : 0ull);
        const int wl = (w0 + 63 < n ? w0 + 63 : n - 1) / psize;
        unsigned long long sb = 0;
        if (wl != pa) sb = wave_sum_u64(mine != pa ? (unsigned long long)u : 0ull);
        if (lane == 0) {
          if (sa >= (1ull << 32)) {
            misc[kSat] = 1u;
          } else if (sa) {
            const uint32_t old = atomicAdd(&psum[pa], (uint32_t)sa);
            if ((uint32_t)(old + (uint32_t)sa) < old) misc[kSat] = 1u;
          }
          if (wl != pa) {
            if (sb >= (1ull << 32)) {
              misc[kSat] = 1u;
            } else if (sb) {
              const uint32_t old = atomicAdd(&psum[wl], (uint32_t)sb);
              if ((uint32_t)(old + (uint32_t)sb) < old) misc[kSat] = 1u;
            }
          }
        }
      }
    }
    my_umax = wave_max_u32(my_umax);
    if (lane == 0) atomicMax(&misc[kUMax], my_umax);
    __syncthreads();

    // ---- the parameter window ----
    if (tid < nparts) {
      const unsigned long long len = (unsigned long long)(psize - (tid == 0 ? q : 0));
      const unsigned long long S = psum[tid];
      uint32_t lo = 0, hi = 0;
      while (lo < maxp && ((3ull * len) << lo) <= S) ++lo;
      while (hi < maxp && (len << hi) <= S) ++hi;
      atomicMin(&misc[kLo], lo);
      atomicMax(&misc[kHi], hi);
    }
    __syncthreads();
    const bool wide = misc[kUMax] >= kWideU;
    int lo = (int)misc[kLo], hi = (int)misc[kHi];
    if (wide || misc[kSat] != 0u) {
      lo = 0;
      hi = (int)maxp;
    }
    const int W = hi - lo + 1;

    // ---- finest partitions' bit tables (PrcBitTable::from_errors, rice.rs:65-103), one lane per (partition, p) ----
    for (int item = tid; item < nparts * W; item += kOsThreads) {
      const int i = item / W;
      const int pp = lo + item % W;
      const int start = i * psize > q ? i * psize : q;
      const int end = (i + 1) * psize;
      uint32_t acc = 0;
      for (int c0 = start; c0 < end; c0 += 16) {
        const int ce = c0 + 16 < end ? c0 + 16 : end;
        for (int t = c0; t < ce; ++t) acc += ubuf[t] >> pp;
        acc = acc > kMaxBits ? kMaxBits : acc;
      }
      const uint32_t v = acc + 4u + (uint32_t)(end - start) * (uint32_t)(pp + 1);
      tab[i * kTabStride + pp] = v > kMaxBits ? kMaxBits : v;
    }
    __syncthreads();

    // ---- the partition orders, finest first; strict < keeps the finer order (rice.rs:285) ----
    unsigned long long best_bits = ~0ull;
    int best_lvl = 0;
    bool best_r2 = false;
    bool best_clamp = false;
    const int levels = a.rice_finest_only ? 1 : fo + 1;
    for (int k = 0; k < levels; ++k) {
      const int np = nparts >> k;
      if (k > 0) {
        // PrcBitTable::merge (rice.rs:144-152); level k's partition i lives in row i << k
        for (int item = tid; item < np * W; item += kOsThreads) {
          const int i = item / W;
          const int pp = lo + item % W;
          const uint32_t x = tab[(i << k) * kTabStride + pp];
          const uint32_t y = tab[((2 * i + 1) << (k - 1)) * kTabStride + pp];
          const uint32_t v = x + y - 4u;
          tab[(i << k) * kTabStride + pp] = v > kMaxBits ? kMaxBits : v;
        }
        __syncthreads();
      }
      if (tid < np) {
        uint32_t m = 0xFFFFFFFFu;  // PrcBitTable::minimizer (rice.rs:115-141): min over (bits << 5) | p
        for (int pp = lo; pp <= hi; ++pp) {
          const uint32_t packed = (tab[(tid << k) * kTabStride + pp] << 5) | (uint32_t)pp;
          m = packed < m ? packed : m;
        }
        if ((m >> 5) >= kMaxBits) {  // every entry of 0..max_p saturates: the reference's minimiser picks p = 0
          m = kMaxBits << 5;
          atomicOr(&misc[kClamp], 1u << k);
        }
        pl[tid] = (uint8_t)(m & 31u);
        atomicAdd(&lvl_bits[k], (unsigned long long)(m >> 5));
        if ((m & 31u) > 14u) atomicOr(&misc[kRice2], 1u << k);
      }
      __syncthreads();
      const unsigned long long lb = lvl_bits[k];
      if (lb < best_bits) {
        best_bits = lb;
        best_lvl = k;
        best_r2 = ((misc[kRice2] >> k) & 1u) != 0u;
        best_clamp = ((misc[kClamp] >> k) & 1u) != 0u;
        if ((wide || best_clamp) && tid < np) psel[tid] = pl[tid];  // (each lane its own entry)
      }
    }

    // ---- Lpc::count_bits (bitrepr.rs:492-499, 533-544) ----
    const int nb = nparts >> best_lvl;
    const unsigned long long wq = (unsigned long long)q;
    unsigned long long key;
    if (!wide && !best_clamp) {
      // no entry of the chosen level saturates or wraps: code_bits is the exact sum, and the residual's bits are
      // 2 + 4 + nb * (4 or 5) + quotients + remainders = 6 + code_bits (+ nb with the 5-bit parameters)
      key = 8ull + bps * wq + 4ull + 5ull + prec * wq + 6ull + best_bits + (best_r2 ? (unsigned long long)nb : 0ull);
    } else {
      __syncthreads();  // (psel complete)
      const int pb = psize << best_lvl;
      unsigned long long s = 0;
      for (int t = q + tid; t < n; t += kOsThreads) s += (unsigned long long)(ubuf[t] >> psel[t / pb]);
      s = wave_sum_u64(s);
      if (lane == 0) atomicAdd(&acc64[0], s);
      __syncthreads();
      const unsigned long long sum_q = acc64[0];
      unsigned long long sum_p = 0;
      for (int i = 0; i < nb; ++i) sum_p += psel[i];
      const unsigned long long rbits = 6ull + (unsigned long long)nb * (best_r2 ? 5ull : 4ull) + sum_q +
                                       (unsigned long long)(n - q) + (sum_p * (unsigned long long)pb - wq * psel[0]);
      key = 8ull + bps * wq + 4ull + 5ull + prec * wq + rbits;
    }
    if (key < best_key) {  // strict: the lower candidate -- window, then order, then the higher precision -- wins a tie
      best_key = key;
      best_c = (uint32_t)cand + 1u;
    }
  }
  if (tid == 0) a.best[sf] = best_c;
}

// One slice of subframes of the flagged batch: racc [n][W][33], cand [n][C][36], best [n] in the scratch; pred, lpc_coefs and
// autocorr already offset to the slice's first subframe.
struct SliceArgs {
  const double* racc;
  double* refl;  // the order guess: k_o of every candidate [n][C], else nullptr
  int32_t* cand;
  uint32_t* best;
  int32_t* pred;
  double* lpc_coefs;
  double* autocorr;
  uint32_t n_subframes;
  uint32_t W, P, Pc, Q, precision;
};

template <int MAXP>
hipError_t launch_levinson_and_pick(bool pick, const SliceArgs& s, hipStream_t stream) {
  if (!pick) {
    const size_t items = (size_t)s.n_subframes * s.W * s.Pc;
    if (s.refl)
      hipLaunchKernelGGL((order_levinson_kernel<MAXP, true>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, stream,
                         s.racc, s.n_subframes, s.W, s.P, s.Pc, s.Q, s.precision, s.cand, s.refl);
    else
      hipLaunchKernelGGL((order_levinson_kernel<MAXP, false>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, stream,
                         s.racc, s.n_subframes, s.W, s.P, s.Pc, s.Q, s.precision, s.cand, s.refl);
  } else {
    hipLaunchKernelGGL(order_pick_kernel<MAXP>, dim3((s.n_subframes + 63) / 64), dim3(64), 0, stream, s.racc, s.n_subframes,
                       s.W, s.P, s.Pc, s.Q, s.precision, s.best, s.pred, s.lpc_coefs, s.autocorr);
  }
  return hipGetLastError();
}

hipError_t levinson_bucket(bool pick, const SliceArgs& s, hipStream_t stream) {
  const uint32_t P = s.P;
  if (P <= 8) return launch_levinson_and_pick<8>(pick, s, stream);
  if (P <= 12) return launch_levinson_and_pick<12>(pick, s, stream);
  if (P <= 16) return launch_levinson_and_pick<16>(pick, s, stream);
  if (P <= 24) return launch_levinson_and_pick<24>(pick, s, stream);
  return launch_levinson_and_pick<32>(pick, s, stream);
}

size_t bytes_per_subframe(uint32_t lpc_order, const SearchShape& shape) {
  const size_t W = shape.n_windows, G = W * (shape.search_orders ? lpc_order : 1u), C = G * shape.n_precisions;
  return W * 33 * sizeof(double) + (shape.guess_orders ? G * sizeof(double) : 0) + C * kCandWords * 4 + 4;
}

// subframes per slice: as many as kSearchScratchCap holds, whole stereo frames (a multiple of 4), at least 4
size_t slice_subframes(size_t n, uint32_t lpc_order, const SearchShape& shape) {
  size_t k = kSearchScratchCap / bytes_per_subframe(lpc_order, shape);
  k = k < 4 ? 4 : (k & ~static_cast<size_t>(3));
  return n < k ? n : k;
}

}  // namespace

size_t order_search_scratch_bytes(uint32_t n_subframes, uint32_t lpc_order, const SearchShape& shape) {
  return slice_subframes(n_subframes, lpc_order, shape) * bytes_per_subframe(lpc_order, shape);
}

hipError_t launch_order_search(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, uint32_t nightly,
                               const SearchShape& shape, void* scratch, hipStream_t stream, uint32_t* n_slices) {
  if (n_slices) *n_slices = 0;
  if (a.n_subframes == 0) return hipSuccess;
  if (a.split_scratch == nullptr || scratch == nullptr || a.lpc_order < 1 || a.lpc_order > 32 || a.block_size < 64 ||
      a.block_size > 32767 || shape.n_windows < 1 || shape.n_windows > kMaxSearchWindows || shape.guess_orders > 32 ||
      (shape.guess_orders && !shape.search_orders) || shape.n_precisions < 1 || shape.n_precisions > a.precision)
    return hipErrorInvalidValue;
  const size_t n = a.n_subframes;
  const uint32_t W = shape.n_windows;
  const uint32_t Pc = shape.search_orders ? a.lpc_order : 1u;
  const uint32_t Q = shape.n_precisions;
  const uint32_t G = W * Pc, C = G * Q;
  const size_t slice = slice_subframes(n, a.lpc_order, shape);
  int32_t* pred = reinterpret_cast<int32_t*>(reinterpret_cast<double*>(a.split_scratch) + n * 33);
  double* racc = static_cast<double*>(scratch);
  double* refl = shape.guess_orders ? racc + slice * W * 33 : nullptr;
  int32_t* cand = reinterpret_cast<int32_t*>(racc + slice * W * 33 + (refl ? slice * G : 0));
  uint32_t* best = reinterpret_cast<uint32_t*>(cand + slice * C * kCandWords);

  const bool lds_u = search_lds_bytes(a.block_size, true) <= 160 * 1024;
  const size_t smem = search_lds_bytes(a.block_size, lds_u);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  if (!lds_u && a.residual == nullptr) return hipErrorInvalidValue;
  hipError_t err;
  if (lds_u) {
    static DynamicLdsOptIn opt_in;
    if ((err = opt_in.ensure(reinterpret_cast<const void*>(order_search_kernel<true>), smem)) != hipSuccess) return err;
  } else {
    static DynamicLdsOptIn opt_in;
    if ((err = opt_in.ensure(reinterpret_cast<const void*>(order_search_kernel<false>), smem)) != hipSuccess) return err;
  }
  for (size_t sf0 = 0; sf0 < n; sf0 += slice) {
    const uint32_t ns = static_cast<uint32_t>(n - sf0 < slice ? n - sf0 : slice);
    if (n_slices) ++*n_slices;
    // (stereo slices are whole frames: frame f's two channels at samples + 2 f stride)
    const int32_t* samples = a.samples + (a.stereo ? sf0 / 2 : sf0) * a.stride;
    // 1. R[0..P] of every window in the stable build's order (or nightly's)
    for (uint32_t j = 0; j < W; ++j) {
      AcorrRefArgs r{};
      r.samples = samples;
      r.stride = a.stride;
      r.block_size = a.block_size;
      r.n_subframes = ns;
      r.stereo = a.stereo;
      r.window = shape.windows[j];
      r.lpc_order = a.lpc_order;
      r.nightly = nightly;
      r.out = racc + j * 33;
      r.out_stride = W * 33;
      if ((err = launch_acorr_reference(r, stream)) != hipSuccess) return err;
    }
    SliceArgs sl{};
    sl.racc = racc;
    sl.refl = refl;
    sl.cand = cand;
    sl.best = best;
    sl.pred = pred + sf0 * kCandWords;
    sl.lpc_coefs = a.lpc_coefs ? a.lpc_coefs + sf0 * 32 : nullptr;
    sl.autocorr = a.autocorr ? a.autocorr + sf0 * 33 : nullptr;
    sl.n_subframes = ns;
    sl.W = W;
    sl.P = a.lpc_order;
    sl.Pc = Pc;
    sl.Q = Q;
    sl.precision = a.precision;
    // 2. every candidate's predictor
    if ((err = levinson_bucket(false, sl, stream)) != hipSuccess) return err;
    if (refl) {  // 2b. the order guess: all but (0, P) and every window's guesses struck from the search
      const size_t items = (size_t)ns * W;
      hipLaunchKernelGGL(order_guess_kernel, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, stream, racc, refl, cand,
                         ns, W, a.lpc_order, Q, a.precision, a.block_size, a.bps ? a.bps + sf0 : nullptr, a.bps_uniform,
                         a.stereo, shape.guess_orders,
                         shape.guess_trace ? static_cast<order_guess::Guess*>(shape.guess_trace) + sf0 * W : nullptr);
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    // 3. the search
    OrderSearchArgs s{};
    s.samples = samples;
    s.stride = a.stride;
    s.block_size = a.block_size;
    s.n_subframes = ns;
    s.stereo = a.stereo;
    s.bps = a.bps ? a.bps + sf0 : nullptr;
    s.bps_uniform = a.bps_uniform;
    s.lpc_order = a.lpc_order;
    s.n_cand = C;
    s.max_rice_parameter = a.max_rice_parameter;
    s.rice_finest_only = a.rice_finest_only;
    s.cand = cand;
    s.best = best;
    s.residual = a.residual ? a.residual + sf0 * a.residual_stride : nullptr;
    s.residual_stride = a.residual_stride;
    if (lds_u) hipLaunchKernelGGL(order_search_kernel<true>, dim3(ns), dim3(kOsThreads), smem, stream, s);
    else hipLaunchKernelGGL(order_search_kernel<false>, dim3(ns), dim3(kOsThreads), smem, stream, s);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    // 4. the chosen candidate's predictor record (+ unquantised coefficients, + its window's R[])
    if ((err = levinson_bucket(true, sl, stream)) != hipSuccess) return err;
  }
  // 5. records and residual rows by the unflagged stage-3 kernels (as behind direct_mse_kernel)
  QlpcKernelArgs s3 = a;
  s3.reference_order = 0;
  s3.certify = 0;
  s3.cert_subwave = 0;
  s3.integer_parity_only = 0;
  s3.direct_mse = 0;
  s3.sumabs_in = nullptr;
  s3.sumabs_scratch = nullptr;
  return launch_stage3(s3, pred, bigblock_shape_eligible(a), plan, stream);
}

}  // namespace flacenc_hip
