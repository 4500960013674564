// rice_escape.cpp -- FLACENC_HIP_FLAG_RICE_ESCAPE (include/flacenc_hip.h): a post-pass over
// candidate records and their residual rows.  One workgroup per row repeats the reference's partitioned-Rice search
// (PrcParameterFinder::find, rice.rs:246-298: a 32-entry bit table per finest partition, log2 merges) with one more
// choice per partition -- the raw (escaped) form of RFC 9639 9.2.7.1 at the partition's own width -- and rewrites the
// record's Rice fields when some partition of the chosen level escapes.  A record in which none does is not touched.
//
// Tables: bits[p] = min(S_p, M) + 4 + cnt * (p + 1) clamped to M = 2^27 - 1, S_p the sum of z >> p with wrapping u32
// adds and a clamp to M after every 16 samples counted from the partition's start (PrcBitTable::from_errors).  While
// every z of the row is below 2^26 no add wraps, the chunked clamp equals one clamp of the true sum, and a partition's
// samples may be split over threads: partial sums, each clamped, are added in LDS (at most 32 per entry: below 2^32) and
// clamped once more.  A row with a larger z is summed again, one thread per (partition, p), literally.
#include "rice_escape.h"

#include "rice_escape_core.h"

namespace flacenc_hip {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kRow = 33;                  // table row pitch in words: 32 entries + 1 (LDS banks)
constexpr uint32_t kMaxBits = (1u << 27) - 1u;  // MAX_P_TO_BITS, rice.rs:51
constexpr uint32_t kMaxSegments = 32;

__device__ __forceinline__ uint32_t zigzag(int32_t v) {  // rice::encode_signbit, rice.rs:169-171
  return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31);
}

// samples of partition q at partition length `len`: [max(q * len, order), (q + 1) * len)
__device__ __forceinline__ uint32_t part_count(uint32_t q, uint32_t len, uint32_t order) {
  const uint32_t lo = q * len, hi = lo + len;
  return hi - (lo > order ? lo : (order < hi ? order : hi));
}

__global__ void __launch_bounds__(kThreads) rice_escape_kernel(RiceEscapeArgs a) {
  __shared__ uint32_t tab_a[FLACENC_HIP_MAX_RICE_PARTITIONS * kRow];
  __shared__ uint32_t tab_b[(FLACENC_HIP_MAX_RICE_PARTITIONS / 2) * kRow];
  __shared__ int32_t lo_s[2][FLACENC_HIP_MAX_RICE_PARTITIONS], hi_s[2][FLACENC_HIP_MAX_RICE_PARTITIONS];
  __shared__ uint32_t rice_cur[FLACENC_HIP_MAX_RICE_PARTITIONS], rice_best[FLACENC_HIP_MAX_RICE_PARTITIONS];
  __shared__ uint8_t ps_cur[FLACENC_HIP_MAX_RICE_PARTITIONS], ps_best[FLACENC_HIP_MAX_RICE_PARTITIONS];
  __shared__ unsigned long long acc[4];  // 0: the level's cost; 1: old residual bits; 2: new count bits; 3: sum of quotients
  __shared__ uint32_t wide_row;

  const uint32_t tid = threadIdx.x;
  flacenc_hip_subframe_params* rec = a.params + blockIdx.x;
  const uint32_t n = a.block_size;
  if (rec->status != 0 || n < FLACENC_HIP_MIN_BLOCK_SIZE) return;  // (uniform)
  const int32_t* __restrict__ e = a.residual + (size_t)blockIdx.x * a.residual_stride;
  const uint32_t order = rec->order;

  // finest_partition_order(n, max(64, order)), rice.rs:157-165
  uint32_t finest;
  {
    const uint32_t min_part = order > 64u ? order : 64u;
    const uint32_t splits = n / min_part;  // >= 1
    const uint32_t by_size = 31u - (uint32_t)__builtin_clz(splits);
    const uint32_t by_zeros = (uint32_t)__builtin_ctz(n);
    finest = by_size < by_zeros ? by_size : by_zeros;
    finest = finest < 8u ? finest : 8u;
  }
  const uint32_t nparts = 1u << finest, psize = n >> finest;

  // ---- the finest partitions' tables and extremes ----
  uint32_t nseg = (psize + 255u) / 256u;
  nseg = nseg < kMaxSegments ? nseg : kMaxSegments;
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t i = tid; i < nparts * kRow; i += kThreads) tab_a[i] = 0u;
    for (uint32_t q = tid; q < nparts; q += kThreads) {
      lo_s[0][q] = 0x7FFFFFFF;
      hi_s[0][q] = (int32_t)0x80000000;
    }
    if (tid == 0) wide_row = 0u;
    __syncthreads();
    const uint32_t seg_len = (((psize + nseg - 1u) / nseg) + 15u) & ~15u;
    const uint32_t tasks = nparts * nseg * 32u;
    for (uint32_t task = tid; task < tasks; task += kThreads) {
      const uint32_t p = task & 31u, qs = task >> 5;
      const uint32_t q = qs / nseg, s = qs - q * nseg;
      const uint32_t part_lo = q * psize, part_hi = part_lo + psize;
      uint32_t t0 = part_lo + s * seg_len, t1 = t0 + seg_len;
      t0 = t0 > order ? t0 : order;
      t1 = t1 < part_hi ? t1 : part_hi;
      if (t0 >= t1) continue;
      uint32_t sum = 0u, zmax = 0u;
      int32_t mn = 0x7FFFFFFF, mx = (int32_t)0x80000000;
      for (uint32_t c0 = t0; c0 < t1; c0 += 16u) {
        const uint32_t c1 = c0 + 16u < t1 ? c0 + 16u : t1;
        for (uint32_t t = c0; t < c1; ++t) {
          const int32_t v = e[t];
          const uint32_t z = zigzag(v);
          sum += z >> p;
          zmax |= z;
          mn = v < mn ? v : mn;
          mx = v > mx ? v : mx;
        }
        sum = sum < kMaxBits ? sum : kMaxBits;
      }
      atomicAdd(&tab_a[q * kRow + p], sum);
      if (p == 0u) {
        atomicMin(&lo_s[0][q], mn);
        atomicMax(&hi_s[0][q], mx);
        if (zmax >> 26) wide_row = 1u;
      }
    }
    __syncthreads();
    const bool again = wide_row != 0u && nseg > 1u;
    __syncthreads();  // (wide_row is cleared at the top of the next pass)
    if (!again) break;
    nseg = 1u;
  }
  for (uint32_t i = tid; i < nparts * 32u; i += kThreads) {
    const uint32_t q = i >> 5, p = i & 31u;
    uint32_t v = tab_a[q * kRow + p];
    v = v < kMaxBits ? v : kMaxBits;
    v += 4u + part_count(q, psize, order) * (p + 1u);
    tab_a[q * kRow + p] = v < kMaxBits ? v : kMaxBits;
  }
  if (tid == 0) acc[0] = 0ull;
  __syncthreads();

  // ---- the walk over the levels, rice.rs:277-291, on sum_q min(R, E) ----
  unsigned long long best_cost = 0ull;
  uint32_t best_level = finest;
  uint32_t* cur = tab_a;
  uint32_t* nxt = tab_b;
  uint32_t side = 0u;
  for (uint32_t level = finest;; --level) {
    const uint32_t np = 1u << level, len = n >> level;
    if (tid < np) {
      uint32_t packed = 0xFFFFFFFFu;  // PrcBitTable::minimizer: smallest (bits << 5 | p) over p <= max_p
      for (uint32_t p = 0; p <= a.max_rice_parameter; ++p) {
        const uint32_t v = (cur[tid * kRow + p] << 5) | p;
        packed = v < packed ? v : packed;
      }
      const uint32_t rice_cost = packed >> 5, rice_param = packed & 31u;
      const uint32_t cnt = part_count(tid, len, order);
      const uint32_t w = rice_escape::raw_width(lo_s[side][tid], hi_s[side][tid]);
      ps_cur[tid] = (uint8_t)rice_escape::chosen_param(rice_cost, rice_param, cnt, w);
      rice_cur[tid] = rice_cost;
      atomicAdd(&acc[0], (unsigned long long)rice_escape::chosen_cost(rice_cost, cnt, w));
    }
    __syncthreads();
    const unsigned long long cost = acc[0];
    if (level == finest || cost < best_cost) {  // (uniform)
      best_cost = cost;
      best_level = level;
      if (tid < np) {
        ps_best[tid] = ps_cur[tid];
        rice_best[tid] = rice_cur[tid];
      }
    }
    if (level == 0u || a.finest_only) break;
    __syncthreads();
    if (tid == 0) acc[0] = 0ull;
    for (uint32_t i = tid; i < (np >> 1) * 32u; i += kThreads) {  // PrcBitTable::merge(.., 4)
      const uint32_t q = i >> 5, p = i & 31u;
      const uint32_t v = cur[(2u * q) * kRow + p] + cur[(2u * q + 1u) * kRow + p] - 4u;
      nxt[q * kRow + p] = v < kMaxBits ? v : kMaxBits;
    }
    for (uint32_t q = tid; q < (np >> 1); q += kThreads) {
      const int32_t l0 = lo_s[side][2u * q], l1 = lo_s[side][2u * q + 1u];
      const int32_t h0 = hi_s[side][2u * q], h1 = hi_s[side][2u * q + 1u];
      lo_s[side ^ 1u][q] = l0 < l1 ? l0 : l1;
      hi_s[side ^ 1u][q] = h0 > h1 ? h0 : h1;
    }
    side ^= 1u;
    uint32_t* const t = cur;
    cur = nxt;
    nxt = t;
    __syncthreads();
  }
  __syncthreads();

  // ---- the record: untouched unless a partition of the chosen level escapes ----
  const uint32_t np = 1u << best_level, len = n >> best_level;
  const bool mine_marked = tid < np && rice_escape::is_marked(ps_best[tid]);
  if (!__syncthreads_or(mine_marked ? 1 : 0)) return;

  // everything in front of the residual: the old count less the old residual (bitrepr.rs:533-544)
  const uint32_t old_level = rec->rice_order;
  const uint32_t old_np = 1u << old_level, old_len = n >> old_level;
  const unsigned long long old_bits = rec->subframe_bits, old_quotients = rec->sum_quotients;
  if (tid < 4) acc[tid] = 0ull;
  __syncthreads();
  uint32_t old_rice2 = 0u;
  if (tid < old_np) {
    const uint32_t k = rec->rice_params[tid];
    old_rice2 = k > 14u ? 1u : 0u;
    atomicAdd(&acc[1], (unsigned long long)part_count(tid, old_len, order) * (k + 1u));
  }
  old_rice2 = __syncthreads_or((int)old_rice2) ? 1u : 0u;
  uint32_t rice2 = 0u, clamped = 0u;
  if (tid < np) {
    const uint32_t par = ps_best[tid], cnt = part_count(tid, len, order);
    rice2 = rice_escape::wants_rice2(par) ? 1u : 0u;
    atomicAdd(&acc[2], (unsigned long long)rice_escape::partition_body_bits(par, cnt, 0ull));
    if (!rice_escape::is_marked(par)) {
      // an entry below the clamp is exact at every level (a merged entry is no smaller than its children's)
      const uint32_t r = rice_best[tid];
      if (r >= kMaxBits) clamped = 1u;
      else atomicAdd(&acc[3], (unsigned long long)(r - 4u - cnt * (par + 1u)));
    }
  }
  rice2 = __syncthreads_or((int)rice2) ? 1u : 0u;
  if (__syncthreads_or((int)clamped)) {  // the exact sum of quotients from the row itself
    if (tid == 0) acc[3] = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (uint32_t t = order + tid; t < n; t += kThreads) {
      const uint32_t par = ps_best[t / len];
      if (!rice_escape::is_marked(par)) mine += zigzag(e[t]) >> par;
    }
    atomicAdd(&acc[3], mine);
    __syncthreads();
  }
  const unsigned long long old_residual = 6ull + (unsigned long long)old_np * (old_rice2 ? 5u : 4u) + old_quotients + acc[1];
  const unsigned long long new_residual = 6ull + (unsigned long long)np * (rice2 ? 5u : 4u) + acc[2] + acc[3];
  rec->rice_params[tid] = tid < np ? ps_best[tid] : (uint8_t)0;
  if (tid == 0) {
    rec->rice_order = (uint8_t)best_level;
    rec->code_bits = best_cost;
    rec->sum_quotients = acc[3];
    rec->subframe_bits = old_bits - old_residual + new_residual;
  }
}

}  // namespace

hipError_t launch_rice_escape(const RiceEscapeArgs& a, hipStream_t stream) {
  if (a.n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(rice_escape_kernel, dim3(a.n_rows), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace flacenc_hip
