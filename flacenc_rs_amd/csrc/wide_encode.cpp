// wide_encode.cpp -- the wide encode path on the device: rows of 8..32-bit samples in, FLAC
// frame bytes and lengths out, by the rule of wide_encode_core.h.  Two kernels:
//   wide_decide_kernel  one workgroup per (frame, role): encode_subframe over Constant, Verbatim and the fixed predictors
//                       of order 0..4 with the exhaustive partitioned-Rice search; writes a SubRecord
//   wide_write_kernel   one workgroup per frame: the stereo decision, the header, the subframes with fields up to 33 bits
//                       wide, the CRC-16; the residual is recomputed from the samples
// Nothing here touches the analysis kernels, the packers or their records.
#include "api_internal.h"
#include "wide_encode_core.h"

namespace flacenc_hip {
namespace {

using namespace wideenc;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = 512;  // samples whose u[] is staged at a time: one run of 64 per half-wave

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int mask) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), mask, 64));
  const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v >> 32)), mask, 64));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

struct DecideShared {
  Tables tab;
  uint32_t u[kChunk];
  unsigned long long lbits[MAX_PARTS];
  uint8_t lparams[MAX_PARTS], cur_params[MAX_PARTS], best_params[MAX_PARTS];
  unsigned long long red_or[kThreads / 64];
  long long red_min[kThreads / 64], red_max[kThreads / 64];
  unsigned long long total;
  int ineligible;
};

// Every decision value below (k, the keys, the bit counts, the orders) is computed by all threads from shared words that
// are complete at the barrier before: the branches on them are uniform.
__global__ void __launch_bounds__(kThreads) wide_decide_kernel(WideEncodeArgs a) {
  __shared__ DecideShared s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t roles = roles_of(a.channels), n = a.block_size;
  const Config cfg = a.cfg;
  const uint32_t max_p = cfg.max_rice_parameter < MAX_PARAMS - 1 ? cfg.max_rice_parameter : MAX_PARAMS - 1;
  const uint32_t max_order = cfg.fixed_max_order < 4 ? cfg.fixed_max_order : 4;
  const uint32_t F = finest_order(n), parts = 1u << F, size = n >> F;
  const uint64_t jobs = static_cast<uint64_t>(a.n_frames) * roles;
  for (uint64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const uint32_t f = static_cast<uint32_t>(job / roles), role = static_cast<uint32_t>(job % roles);
    const Rows rows = {a.frames + static_cast<size_t>(f) * a.channels * a.stride, a.stride, a.channels};
    const uint32_t width = role_width(a.channels, role, a.bits_per_sample);
    SubRecord* rec = a.records + job;

    // ---- the role once: OR, minimum, maximum ----
    unsigned long long acc = 0;
    long long mn = INT64_MAX, mx = INT64_MIN;
    for (uint32_t t = tid; t < n; t += kThreads) {
      const long long v = role_sample(rows, role, t);
      acc |= static_cast<unsigned long long>(v);
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      acc |= shfl_xor64(acc, d);
      const long long l2 = static_cast<long long>(shfl_xor64(static_cast<unsigned long long>(mn), d));
      const long long h2 = static_cast<long long>(shfl_xor64(static_cast<unsigned long long>(mx), d));
      mn = l2 < mn ? l2 : mn;
      mx = h2 > mx ? h2 : mx;
    }
    if (lane == 0) {
      s.red_or[wave] = acc;
      s.red_min[wave] = mn;
      s.red_max[wave] = mx;
    }
    __syncthreads();
    for (uint32_t w2 = 0; w2 < kThreads / 64; ++w2) {
      acc |= s.red_or[w2];
      mn = s.red_min[w2] < mn ? s.red_min[w2] : mn;
      mx = s.red_max[w2] > mx ? s.red_max[w2] : mx;
    }
    const bool constant = mn == mx;
    if (cfg.use_constant && constant) {
      if (tid == 0) constant_record(mn, width, rec);
    } else {
      const uint32_t k = wasted_of(acc, constant, cfg), w = width - k;
      bool have = false;
      unsigned long long best_key = 0, best_code_bits = 0;
      uint32_t best_order = 0, best_porder = 0;
      for (uint32_t o = 0; n >= MIN_PREDICTION && cfg.use_fixed && o <= max_order; ++o) {
        for (uint32_t i = tid; i < parts * LOW_PARAMS; i += kThreads) (&s.tab.lo[0][0])[i] = 0;
        for (uint32_t i = tid; i < parts * (MAX_PARAMS - LOW_PARAMS); i += kThreads) (&s.tab.hi[0][0])[i] = 0;
        if (tid == 0) s.ineligible = 0;
        __syncthreads();
        int bad = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += kChunk) {
          for (uint32_t i = tid; i < kChunk; i += kThreads) {
            const uint32_t t = c0 + i;
            uint32_t u = 0;  // the warm-up and what lies past the block add nothing to a sum
            if (t < n && t >= o) {
              const int64_t e = fixed_error(rows, role, k, o, t);
              if (codable(e)) u = zigzag(e);
              else s.ineligible = 1;
            }
            s.u[i] = u;
          }
          __syncthreads();
          bad = s.ineligible;
          // a half-wave per run of 64 samples, a lane per parameter; the run lies in two partitions at most (size >= 64)
          const uint32_t p = tid & 31u, t0 = c0 + 64u * (tid >> 5);
          if (!bad && p < MAX_PARAMS && t0 < n) {
            const uint32_t t1 = t0 + 64u < n ? t0 + 64u : n;
            const uint32_t q0 = t0 / size;
            const uint32_t tb = (q0 + 1u) * size < t1 ? (q0 + 1u) * size : t1;
            unsigned long long sa = 0, sb = 0;
            for (uint32_t t = t0; t < tb; ++t) sa += s.u[t - c0] >> p;
            for (uint32_t t = tb; t < t1; ++t) sb += s.u[t - c0] >> p;
            if (p < LOW_PARAMS) {
              if (sa) atomicAdd(&s.tab.lo[q0][p], sa);
              if (sb) atomicAdd(&s.tab.lo[q0 + 1u][p], sb);
            } else {
              if (sa) atomicAdd(&s.tab.hi[q0][p - LOW_PARAMS], static_cast<uint32_t>(sa));
              if (sb) atomicAdd(&s.tab.hi[q0 + 1u][p - LOW_PARAMS], static_cast<uint32_t>(sb));
            }
          }
          __syncthreads();
          if (bad) break;
        }
        if (bad) continue;  // RFC 9639 section 9.2.7.3: this order cannot be coded
        unsigned long long cur_bits = 0;
        uint32_t cur_porder = 0;
        for (uint32_t level = F;; --level) {
          const uint32_t lparts = 1u << level, step = 1u << (F - level);
          if (tid < lparts) {
            uint32_t p;
            s.lbits[tid] = best_parameter(s.tab, tid * step, (n >> level) - (tid == 0 ? o : 0u), max_p, &p);
            s.lparams[tid] = static_cast<uint8_t>(p);
          }
          __syncthreads();
          if (wave == 0) {
            unsigned long long v = 0;
            for (uint32_t j = lane; j < lparts; j += 64) v += s.lbits[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) v += shfl_xor64(v, d);
            if (lane == 0) s.total = v;
          }
          __syncthreads();
          const unsigned long long total = s.total;
          if (level == F || total < cur_bits) {
            cur_bits = total;
            cur_porder = level;
            if (tid < lparts) s.cur_params[tid] = s.lparams[tid];
          }
          if (level == 0) break;
          for (uint32_t i = tid; i < (lparts / 2) * MAX_PARAMS; i += kThreads) {
            const uint32_t j = i / MAX_PARAMS;
            merge_pair(s.tab, 2 * j * step, (2 * j + 1) * step, i % MAX_PARAMS);
          }
          __syncthreads();
        }
        const unsigned long long key = static_cast<unsigned long long>(w) * o + cur_bits;
        if (!have || key < best_key) {
          have = true;
          best_key = key;
          best_code_bits = cur_bits;
          best_order = o;
          best_porder = cur_porder;
          if (tid < (1u << cur_porder)) s.best_params[tid] = s.cur_params[tid];
        }
      }
      __syncthreads();
      if (tid == 0) finish_record(have, best_key, best_code_bits, best_order, best_porder, s.best_params, n, w, k, rec);
    }
    __syncthreads();
  }
}

struct AtomicOr {
  __device__ void operator()(uint32_t* w, uint32_t v) const { atomicOr(w, v); }
};

struct WriteShared {
  uint32_t chosen[8];
  unsigned long long start[9];
  uint32_t header_len;
  uint8_t header[16];
  uint32_t wave_total[kThreads / 64], crc[kThreads / 64];
  uint32_t bad;
};

// The frame is built in its slot with word-wide atomic ORs on zeroed words: a field's position is known from a prefix
// sum, not its neighbours.  The slot's words are zeroed, read back for the CRC and written only with device-scope atomics,
// fenced at the barriers between the three steps.
__global__ void __launch_bounds__(kThreads) wide_write_kernel(WideEncodeArgs a) {
  __shared__ WriteShared s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t roles = roles_of(a.channels), n = a.block_size;
  const AtomicOr aor;
  for (uint32_t f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
    const Rows rows = {a.frames + static_cast<size_t>(f) * a.channels * a.stride, a.stride, a.channels};
    const SubRecord* recs = a.records + static_cast<size_t>(f) * roles;
    uint32_t* words = reinterpret_cast<uint32_t*>(a.out + static_cast<size_t>(f) * a.out_stride);
    if (tid == 0) {
      uint32_t tag = a.channels - 1u;
      for (uint32_t ch = 0; ch < a.channels; ++ch) s.chosen[ch] = ch;
      if (a.channels == 2) {
        const unsigned long long b[4] = {recs[0].bits, recs[1].bits, recs[2].bits, recs[3].bits};
        tag = stereo_choice(b, a.cfg, s.chosen);
      }
      s.header_len = write_header(n, a.sample_rate, a.bits_per_sample, tag, a.first_frame_number + f * a.frame_number_step, s.header);
      unsigned long long pos = 8ull * s.header_len;
      for (uint32_t ch = 0; ch < a.channels; ++ch) {
        s.start[ch] = pos;
        pos += recs[s.chosen[ch]].bits;
      }
      s.start[a.channels] = pos;
      s.bad = 0;
    }
    __syncthreads();
    const unsigned long long body64 = (s.start[a.channels] + 7) / 8;
    if (body64 + 2u > a.out_stride) {  // (cannot happen: no subframe exceeds Verbatim's bits, which the bound counts)
      if (tid == 0) a.out_len[f] = 0;
      __syncthreads();
      continue;
    }
    const uint32_t body = static_cast<uint32_t>(body64), len = body + 2u;
    // (the slot holds the bytes bound rounded up to 16: whole words up to the frame's end lie inside it)
    for (uint32_t i = tid; i < (len + 3u) / 4u; i += kThreads) __hip_atomic_store(words + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __syncthreads();
    if (tid < s.header_len) put_bits(words, 8ull * tid, s.header[tid], 8, aor);
    for (uint32_t ch = 0; ch < a.channels; ++ch) {
      const uint32_t role = s.chosen[ch];
      const SubRecord& rec = recs[role];
      const uint32_t kind = rec.kind, k = rec.k, order = rec.order;
      const uint32_t w = role_width(a.channels, role, a.bits_per_sample) - k;
      unsigned long long at = s.start[ch] + subframe_head_bits(k);
      if (tid == 0) {
        put_subframe_head(words, s.start[ch], rec, aor);
        if (kind == KIND_CONSTANT) put_bits(words, at, static_cast<uint64_t>(rec.value), w, aor);
      }
      if (kind == KIND_CONSTANT) {
        at += w;
      } else {
        const uint32_t warm = kind == KIND_FIXED ? order : n;
        for (uint32_t t = tid; t < warm; t += kThreads)
          put_bits(words, at + static_cast<unsigned long long>(t) * w, static_cast<uint64_t>(role_sample(rows, role, t) >> k), w, aor);
        at += static_cast<unsigned long long>(warm) * w;
        if (kind == KIND_FIXED) {
          if (tid == 0) put_bits(words, at, (static_cast<uint64_t>(rec.five) << 4) | rec.porder, 6, aor);
          at += 6;
          // a code's length is below the subframe's bits, which are below Verbatim's: 32 bits hold every partial sum
          for (uint32_t c0 = order; c0 < n; c0 += kThreads) {
            const uint32_t t = c0 + tid;
            uint32_t u = 0, p = 0, pb = 0, clen = 0;
            if (t < n) {
              u = zigzag(fixed_error(rows, role, k, order, t));
              clen = code_length(rec, n, t, u, &p, &pb);
            }
            uint32_t incl = clen;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
              const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), d, 64));
              if (lane >= static_cast<uint32_t>(d)) incl += up;
            }
            if (lane == 63) s.wave_total[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w2 = 0; w2 < kThreads / 64; ++w2) {
              before += w2 < wave ? s.wave_total[w2] : 0u;
              all += s.wave_total[w2];
            }
            if (t < n) {
              const unsigned long long pos = at + before + incl - clen;
              put_bits(words, pos, p, pb, aor);
              put_bits(words, pos + clen - p - 1u, (1ull << p) | (u & ((1u << p) - 1u)), p + 1u, aor);
            }
            at += all;
            __syncthreads();
          }
        }
      }
      if (tid == 0 && at != s.start[ch] + rec.bits) s.bad = 1;  // the counted bits are the written bits
    }
    __threadfence();
    __syncthreads();
    // ---- CRC-16: a slice of whole words per thread, shifted to its place, XORed together ----
    const uint32_t per = ((body + kThreads - 1u) / kThreads + 3u) & ~3u;
    const uint32_t b0 = tid * per < body ? tid * per : body, b1 = b0 + per < body ? b0 + per : body;
    uint32_t crc = 0;
    for (uint32_t b = b0; b < b1; b += 4) {
      const uint32_t word = __hip_atomic_load(words + b / 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (uint32_t i = 0; i < 4 && b + i < b1; ++i) {
        crc ^= ((word >> (8u * i)) & 0xFFu) << 8;
        for (int j = 0; j < 8; ++j) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
      }
    }
    if (crc) crc = flacdec::crc16_mulmod(crc, flacdec::crc16_xpow(8u * (body - b1)));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) crc ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(crc), d, 64));
    if (lane == 0) s.crc[wave] = crc;
    __syncthreads();
    if (tid == 0) {
      for (uint32_t w2 = 1; w2 < kThreads / 64; ++w2) crc ^= s.crc[w2];
      put_bits(words, 8ull * body, crc, 16, aor);
      a.out_len[f] = s.bad ? 0u : len;
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_wide_encode(const WideEncodeArgs& a, hipStream_t stream) {
  if (a.n_frames == 0) return hipSuccess;
  const uint64_t jobs = static_cast<uint64_t>(a.n_frames) * wideenc::roles_of(a.channels);
  hipLaunchKernelGGL(wide_decide_kernel, dim3(static_cast<uint32_t>(jobs < (1u << 20) ? jobs : (1u << 20))), dim3(kThreads), 0,
                     stream, a);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  hipLaunchKernelGGL(wide_write_kernel, dim3(a.n_frames < (1u << 20) ? a.n_frames : (1u << 20)), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace flacenc_hip

// The device step on `stream`: what flacenc_hip_encode_pack_frames_wide states, enqueued and not waited for.  The
// stream-level calls run it on their own streams in place of flacenc_hip_encode_pack_(stereo_)frames_async.
int flacenc_hip::encode_pack_frames_wide(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                                         size_t n_frames, uint32_t channels, uint32_t block_size, size_t stride,
                                         uint32_t bits_per_sample, uint32_t sample_rate, uint32_t first_frame_number,
                                         uint32_t frame_number_step, uint8_t* out, size_t out_stride, uint32_t* out_len,
                                         hipStream_t stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!cfg || !frames || !out || !out_len || channels < 1 || channels > 8 || block_size < 1 ||
      block_size > FLACENC_HIP_MAX_BLOCK_SIZE || stride < block_size || bits_per_sample < 8 || bits_per_sample > 32 ||
      n_frames > 0x7FFFFFFFull || (reinterpret_cast<uintptr_t>(out) & 15) || (out_stride & 15) ||
      out_stride < (channels == 2 ? flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample)
                                  : flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample))) {
    h->last_error = "encode_pack_frames_wide: null pointer, channels not in 1..=8, block_size not in 1..=32767, "
                    "bits_per_sample not in 8..=32, or out_stride below the frame bytes bound";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const unsigned long long last = static_cast<unsigned long long>(first_frame_number) +
                                  static_cast<unsigned long long>(n_frames - 1) * frame_number_step;
  if (last >= (1ull << 31)) {
    h->last_error = "encode_pack_frames_wide: frame_number must be below 2^31";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // what the path reads of the config: nothing else is looked at, so a batch may mix depths under one config
  if (cfg->qlpc.max_rice_parameter > FLACENC_HIP_MAX_RICE_PARAMETER || cfg->fixed_max_order > 4) return FLACENC_HIP_ERR_BAD_CONFIG;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t roles = wideenc::roles_of(channels);
  int rc = ensure(h, h->d_wide, n_frames * roles * sizeof(wideenc::SubRecord));
  if (rc != FLACENC_HIP_OK) return rc;
  WideEncodeArgs a;
  a.frames = frames;
  a.stride = stride;
  a.channels = channels;
  a.block_size = block_size;
  a.bits_per_sample = bits_per_sample;
  a.sample_rate = sample_rate;
  a.n_frames = static_cast<uint32_t>(n_frames);
  a.first_frame_number = first_frame_number;
  a.frame_number_step = frame_number_step;
  a.cfg = {cfg->use_constant, cfg->use_fixed, cfg->fixed_max_order, cfg->qlpc.max_rice_parameter, cfg->use_leftside,
           cfg->use_rightside, cfg->use_midside, (cfg->qlpc.flags & FLACENC_HIP_FLAG_WASTED_BITS) ? 1u : 0u};
  a.records = static_cast<wideenc::SubRecord*>(h->d_wide.ptr);
  a.out = out;
  a.out_stride = out_stride;
  a.out_len = out_len;
  HIP_TRY(h, launch_wide_encode(a, stream));
  return FLACENC_HIP_OK;
}

using namespace flacenc_hip;

extern "C" int flacenc_hip_encode_pack_frames_wide(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                                   const int32_t* frames, size_t n_frames, uint32_t channels,
                                                   uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                                   uint32_t sample_rate, uint32_t first_frame_number,
                                                   uint32_t frame_number_step, uint8_t* out, size_t out_stride,
                                                   uint32_t* out_len) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return drained(h, encode_pack_frames_wide(h, cfg, frames, n_frames, channels, block_size, stride, bits_per_sample,
                                            sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len,
                                            h->stream),
                 n_frames == 0);
}
