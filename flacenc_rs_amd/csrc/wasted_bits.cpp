// wasted_bits.cpp -- the kernels of FLACENC_HIP_FLAG_WASTED_BITS (see wasted_bits.h and DESIGN.md section 4.9).
//   wasted_scan_kernel    one wave per frame: OR of every row's samples, stopping as soon as every OR is odd (within
//                         the first 64 samples on ordinary audio: 512 bytes read per stereo frame); k per row and the
//                         list of frames with any k > 0
//   wasted_shift_kernel   the marked frames' rows x >> k and their widths w - k, for the candidate batches
//   wasted_*_decide_kernel  encode_subframe's choice (coding.rs:384-418) over the shifted rows' candidates with the
//                         per-row width and + k bits, try_stereo_coding (coding.rs:493-522) for stereo frames; writes the
//                         marked frames' records (pad = k) and chosen residual rows over the first pass's
#include "wasted_bits.h"

namespace flacenc_hip {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMaxRows = 8;

// row r of a frame whose channels start at x: a stereo role (coding.rs:476-484) or a channel
template <bool STEREO>
__device__ __forceinline__ int32_t row_sample(const int32_t* __restrict__ x, size_t stride, uint32_t r, int t) {
  if (STEREO) {
    const int32_t lv = x[t], rv = x[stride + t];
    return r == 0u ? lv : r == 1u ? rv : r == 2u ? ((lv + rv) >> 1) : (lv - rv);
  }
  return x[(size_t)r * stride + t];
}

__device__ __forceinline__ uint32_t row_width(const WastedArgs& a, uint32_t r) {
  return a.bits_per_sample + ((a.stereo && r == 3u) ? 1u : 0u);  // coding.rs:444
}

template <bool STEREO>
__global__ void __launch_bounds__(kThreads) wasted_scan_kernel(WastedArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (f >= a.n_frames) return;  // (whole waves; no barrier below)
  const uint32_t rows = STEREO ? 4u : a.channels;
  const int n = (int)a.block_size;
  const int32_t* __restrict__ x = a.frames + (size_t)f * a.channels * a.stride;
  uint32_t o[kMaxRows];
  int mn[kMaxRows], mx[kMaxRows];
#pragma unroll
  for (uint32_t r = 0; r < kMaxRows; ++r) {
    o[r] = 0u;
    mn[r] = INT32_MAX;
    mx[r] = INT32_MIN;
  }
  bool odd = false;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const int t = t0 + (int)lane;
    if (t < n) {
#pragma unroll
      for (uint32_t r = 0; r < kMaxRows; ++r) {
        if (r < rows) {
          const int32_t v = row_sample<STEREO>(x, a.stride, r, t);
          o[r] |= (uint32_t)v;
          mn[r] = v < mn[r] ? v : mn[r];
          mx[r] = v > mx[r] ? v : mx[r];
        }
      }
    }
    // every row's OR odd: no row has wasted bits, the rest of the block cannot change that (wave-uniform exit)
    bool all = true;
#pragma unroll
    for (uint32_t r = 0; r < kMaxRows; ++r) {
      const bool any_odd = __any((int)(o[r] & 1u)) != 0;
      if (r < rows) all = all && any_odd;
    }
    if (all) {
      odd = true;
      break;
    }
  }
  uint32_t marked = 0u;
#pragma unroll
  for (uint32_t r = 0; r < kMaxRows; ++r) {
    if (r >= rows) continue;
    uint32_t k = 0u;
    if (!odd) {  // (the whole block was read: the OR and the extremes are complete)
      uint32_t v = o[r];
      int lo = mn[r], hi = mx[r];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        v |= (uint32_t)__shfl_xor((int)v, d, 64);
        const int l2 = __shfl_xor(lo, d, 64), h2 = __shfl_xor(hi, d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      // use_constant and a constant signal: today's Constant, k = 0; an OR of 0 (silence): k = 0
      k = (v == 0u || (a.use_constant && lo == hi)) ? 0u : (uint32_t)__builtin_ctz(v);
    }
    if (lane == 0) a.k[(size_t)f * rows + r] = (uint8_t)k;
    marked |= k;
  }
  if (lane == 0 && marked != 0u) a.list[atomicAdd(a.count, 1u)] = f;
}

// one workgroup per shifted row j = i * rows + r of marked frame list[i]; zero beyond the block up to the row stride
template <bool STEREO>
__global__ void __launch_bounds__(kThreads) wasted_shift_kernel(WastedArgs a) {
  const uint32_t rows = STEREO ? 4u : a.channels;
  const uint32_t j = blockIdx.x;
  const uint32_t i = j / rows, r = j % rows;
  const uint32_t f = a.list[i];
  const uint32_t k = a.k[(size_t)f * rows + r];
  const int n = (int)a.block_size;
  const int32_t* __restrict__ x = a.frames + (size_t)f * a.channels * a.stride;
  int32_t* __restrict__ dst = a.shifted + (size_t)j * a.shifted_stride;
  for (int t = threadIdx.x; t < (int)a.shifted_stride; t += kThreads)
    dst[t] = t < n ? (row_sample<STEREO>(x, a.stride, r, t) >> k) : 0;
  if (threadIdx.x == 0) a.shifted_bps[j] = (uint8_t)(row_width(a, r) - k);
}

// encode_subframe for one row: Constant on the original signal (k = 0), else the shifted signal's candidates at
// width w - k with + k bits (the unary count of the wasted bits); `cand` is the row's candidate index.  This is
// decide_frame's (frame_decide_device.h) and channel_decide_kernel's (frame_decide.cpp) rule with the width and k as
// arguments; those two stay as they are (the fused and big-block kernels compile them), so a change of the rule there
// must be repeated here -- tests/test_gpu_wasted_bits.py holds both paths against the same oracle model.
__device__ __forceinline__ void choose_row(const WastedArgs& a, size_t cand, uint32_t w, uint32_t k, int lo, int hi,
                                           uint32_t* kind_out, unsigned long long* bits_out, uint32_t* k_out) {
  const unsigned long long n = a.block_size;
  if (a.use_constant && lo == hi) {
    *kind_out = FLACENC_HIP_KIND_CONSTANT;
    *bits_out = 8ull + w;  // bitrepr.rs:445
    *k_out = 0u;
    return;
  }
  const unsigned long long bps = w - k;
  const unsigned long long verbatim_bits = 8ull + n * bps;  // datatype.rs:1944
  const bool have_fixed = a.use_fixed && a.fixed_params && a.fixed_keys[cand] < verbatim_bits;  // coding.rs:262, :284
  const unsigned long long fixed_bits = have_fixed ? a.fixed_params[cand].subframe_bits : ~0ull;
  const unsigned long long baseline = fixed_bits < verbatim_bits ? fixed_bits : verbatim_bits;  // coding.rs:403-405
  const bool lpc_ok = a.use_lpc && a.lpc_params && a.lpc_params[cand].status == 0;
  uint32_t kind;
  unsigned long long bits;
  if (lpc_ok && a.lpc_params[cand].subframe_bits < baseline) {
    kind = FLACENC_HIP_KIND_LPC;
    bits = a.lpc_params[cand].subframe_bits;
  } else if (have_fixed && fixed_bits < verbatim_bits) {
    kind = FLACENC_HIP_KIND_FIXED;
    bits = fixed_bits;
  } else {
    kind = FLACENC_HIP_KIND_VERBATIM;
    bits = verbatim_bits;
  }
  *kind_out = kind;
  *bits_out = bits + k;
  *k_out = k;
}

// the chosen candidate's record and residual row (zeros for Constant / Verbatim), all threads
__device__ __forceinline__ void copy_choice(const WastedArgs& a, uint32_t kind, size_t cand,
                                            flacenc_hip_subframe_params* rec, int32_t* dst, int tid) {
  const uint32_t* src_rec = kind == FLACENC_HIP_KIND_LPC     ? reinterpret_cast<const uint32_t*>(a.lpc_params + cand)
                            : kind == FLACENC_HIP_KIND_FIXED ? reinterpret_cast<const uint32_t*>(a.fixed_params + cand)
                                                             : nullptr;
  uint32_t* r = reinterpret_cast<uint32_t*>(rec);
  for (int q = tid; q < (int)(sizeof(flacenc_hip_subframe_params) / 4); q += kThreads) r[q] = src_rec ? src_rec[q] : 0u;
  const int32_t* src = kind == FLACENC_HIP_KIND_LPC     ? a.lpc_residual + cand * a.cand_stride
                       : kind == FLACENC_HIP_KIND_FIXED ? a.fixed_residual + cand * a.cand_stride
                                                        : nullptr;
  for (int t = tid; t < (int)a.block_size; t += kThreads) dst[t] = src ? src[t] : 0;
}

// min / max of `rows` rows over the block, reduced to thread r < rows
template <bool STEREO, int ROWS>
__device__ __forceinline__ void row_extremes(const WastedArgs& a, const int32_t* x, uint32_t row0, uint32_t nrows, int tid,
                                             int (*smin)[kThreads / 64], int (*smax)[kThreads / 64], int* lo, int* hi) {
  int mn[ROWS], mx[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    mn[r] = INT32_MAX;
    mx[r] = INT32_MIN;
  }
  for (int t = tid; t < (int)a.block_size; t += kThreads) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if ((uint32_t)r < nrows) {
        const int v = row_sample<STEREO>(x, a.stride, row0 + r, t);
        mn[r] = v < mn[r] ? v : mn[r];
        mx[r] = v > mx[r] ? v : mx[r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o1 = __shfl_xor(mn[r], d, 64), o2 = __shfl_xor(mx[r], d, 64);
      mn[r] = o1 < mn[r] ? o1 : mn[r];
      mx[r] = o2 > mx[r] ? o2 : mx[r];
    }
    if ((tid & 63) == 0) {
      smin[r][tid >> 6] = mn[r];
      smax[r][tid >> 6] = mx[r];
    }
  }
  __syncthreads();
  if ((uint32_t)tid < nrows) {
    int l = smin[tid][0], h = smax[tid][0];
    for (int w = 1; w < kThreads / 64; ++w) {
      l = smin[tid][w] < l ? smin[tid][w] : l;
      h = smax[tid][w] > h ? smax[tid][w] : h;
    }
    *lo = l;
    *hi = h;
  }
}

// one workgroup per marked stereo frame list[i]
__global__ void __launch_bounds__(kThreads) wasted_frame_decide_kernel(WastedArgs a) {
  __shared__ int smin[4][kThreads / 64], smax[4][kThreads / 64];
  __shared__ unsigned long long sbits[4];
  __shared__ uint32_t skind[4], sk[4], sstatus[4], schoice[3];
  __shared__ int sdc[4];
  const int tid = threadIdx.x;
  const uint32_t i = blockIdx.x;
  const uint32_t f = a.list[i];
  const int32_t* __restrict__ x = a.frames + (size_t)(2u * f) * a.stride;
  int lo = 0, hi = 0;
  row_extremes<true, 4>(a, x, 0u, 4u, tid, smin, smax, &lo, &hi);
  if (tid < 4) {
    const uint32_t role = (uint32_t)tid;
    const size_t cand = (size_t)i * 4 + role;
    uint32_t kind, k;
    unsigned long long bits;
    choose_row(a, cand, row_width(a, role), a.k[(size_t)f * 4 + role], lo, hi, &kind, &bits, &k);
    skind[role] = kind;
    sbits[role] = bits;
    sk[role] = k;
    sdc[role] = lo;
    sstatus[role] = (a.use_lpc && a.lpc_params) ? (uint32_t)a.lpc_params[cand].status : 0u;
  }
  __syncthreads();
  if (tid == 0) {  // try_stereo_coding, coding.rs:493-522; select_channels, datatype.rs:1173-1185
    const unsigned long long bl = sbits[0], br = sbits[1], bm = sbits[2], bs = sbits[3];
    unsigned long long min_bits = bl + br;
    uint32_t assignment = 0;
    if (a.use_leftside && bl + bs < min_bits) {
      min_bits = bl + bs;
      assignment = 1;
    }
    if (a.use_rightside && br + bs < min_bits) {
      min_bits = br + bs;
      assignment = 2;
    }
    if (a.use_midside && bm + bs < min_bits) {
      min_bits = bm + bs;
      assignment = 3;
    }
    schoice[0] = assignment;
    schoice[1] = assignment == 2 ? 3u : (assignment == 3 ? 2u : 0u);
    schoice[2] = (assignment == 0 || assignment == 2) ? 1u : 3u;
    flacenc_hip_stereo_frame_result* fr = a.results + f;
    fr->channel_assignment = (uint8_t)assignment;
    fr->analysis_status = (uint8_t)(sstatus[0] | sstatus[1] | sstatus[2] | sstatus[3]);
    for (int ch = 0; ch < 2; ++ch) {
      const uint32_t role = schoice[1 + ch];
      fr->role[ch] = (uint8_t)role;
      fr->kind[ch] = (uint8_t)skind[role];
      fr->pad[ch] = (uint8_t)sk[role];
      fr->dc_offset[ch] = skind[role] == FLACENC_HIP_KIND_CONSTANT ? sdc[role] : 0;
    }
    fr->bits[0] = bl;
    fr->bits[1] = br;
    fr->bits[2] = bm;
    fr->bits[3] = bs;
  }
  __syncthreads();
  for (int ch = 0; ch < 2; ++ch) {
    const uint32_t role = schoice[1 + ch];
    copy_choice(a, skind[role], (size_t)i * 4 + role, &a.results[f].lpc[ch],
                a.residual + (size_t)(2u * f + (uint32_t)ch) * a.residual_stride, tid);
  }
}

// one workgroup per channel j = i * channels + c of marked Independent frame list[i]
__global__ void __launch_bounds__(kThreads) wasted_channel_decide_kernel(WastedArgs a) {
  __shared__ int smin[1][kThreads / 64], smax[1][kThreads / 64];
  __shared__ uint32_t skind;
  const int tid = threadIdx.x;
  const uint32_t j = blockIdx.x;
  const uint32_t i = j / a.channels, c = j % a.channels;
  const uint32_t f = a.list[i];
  const size_t sf = (size_t)f * a.channels + c;
  const int32_t* __restrict__ x = a.frames + (size_t)f * a.channels * a.stride;
  int lo = 0, hi = 0;
  row_extremes<false, 1>(a, x, c, 1u, tid, smin, smax, &lo, &hi);
  flacenc_hip_channel_result* out = a.chan_results + sf;
  if (tid == 0) {
    uint32_t kind, k;
    unsigned long long bits;
    choose_row(a, j, a.bits_per_sample, a.k[sf], lo, hi, &kind, &bits, &k);
    skind = kind;
    out->kind = (uint8_t)kind;
    out->analysis_status = (uint8_t)((a.use_lpc && a.lpc_params) ? a.lpc_params[j].status : 0);
    out->pad[0] = (uint8_t)k;
    out->pad[1] = 0;
    out->dc_offset = kind == FLACENC_HIP_KIND_CONSTANT ? lo : 0;
    out->bits = bits;
  }
  __syncthreads();
  copy_choice(a, skind, j, &out->params, a.residual + sf * a.residual_stride, tid);
}

}  // namespace

hipError_t launch_wasted_scan(const WastedArgs& a, hipStream_t stream) {
  if (a.n_frames == 0) return hipSuccess;
  const dim3 grid((a.n_frames + kThreads / 64 - 1) / (kThreads / 64));
  if (a.stereo) hipLaunchKernelGGL(wasted_scan_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(wasted_scan_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_wasted_shift(const WastedArgs& a, hipStream_t stream) {
  if (a.m == 0) return hipSuccess;
  const dim3 grid(a.m * wasted_rows(a));
  if (a.stereo) hipLaunchKernelGGL(wasted_shift_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(wasted_shift_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_wasted_decide(const WastedArgs& a, hipStream_t stream) {
  if (a.m == 0) return hipSuccess;
  if (a.stereo) hipLaunchKernelGGL(wasted_frame_decide_kernel, dim3(a.m), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(wasted_channel_decide_kernel, dim3(a.m * a.channels), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace flacenc_hip
