// flac_decode_device.h -- what the decoder's translation units (flac_decode.cpp, stream_index.cpp, flac_decode_streams.cpp,
// flac_decode_ranges.cpp, flac_recover_streams.cpp) share on the device, each written once: the index's constants, workgroup scan, bisection and
// chain walks, and a lane's subframe reconstruction -- its setup, the order-bucket ladder, the sample step, the
// packed-PCM writer and the planar writer.  Included by those five files only.
#ifndef FLAC_DECODE_DEVICE_H_
#define FLAC_DECODE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flac_decode_core.h"
#include "stream_planar_core.h"

namespace flacenc_hip {

constexpr uint32_t kEnd = 0xFFFFFFFEu, kDead = 0xFFFFFFFFu;  // chain sentinels
// the candidate pass: byte positions per lane and per workgroup of 256
constexpr uint32_t kPosPerThread = 16, kPosPerBlock = 256 * kPosPerThread;

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

// a kernel launch that counts itself in plan[0]
#define COUNTED_LAUNCH(plan, ...)      \
  do {                                 \
    hipLaunchKernelGGL(__VA_ARGS__);   \
    ++(plan)[0];                       \
  } while (0)

// ---------------------------------------------------------------- index
// exclusive scan of v over the workgroup (256 threads); returns the exclusive prefix, *total = the sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t x = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  *total = sh[255];
  const uint32_t incl = sh[threadIdx.x];
  __syncthreads();
  return incl - v;
}

// the first candidate of [lo, n) at or behind byte x; n if there is none (positions ascend)
__device__ inline uint32_t lower_bound(const uint64_t* cand_pos, uint32_t lo, uint32_t n, uint64_t x) {
  uint32_t hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cand_pos[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the verified candidate (skim and CRC-16 passed) of [lo, n) that starts at byte x, kDead if there is none
__device__ inline uint32_t verified_at(const uint64_t* cand_pos, const flacdec::FrameRec* recs, uint32_t lo, uint32_t n,
                                       uint64_t x) {
  const uint32_t i = lower_bound(cand_pos, lo, n, x);
  return i < n && cand_pos[i] == x && recs[i].status == 0 ? i : kDead;
}

// the chain from `root` by binary lifting over the jump levels (level k at jump + k * capacity): its last node and the
// number of its nodes
struct ChainEnd {
  uint32_t last;
  uint64_t count;
};
__device__ inline ChainEnd walk_chain(const uint32_t* jump, uint32_t levels, uint32_t capacity, uint32_t root) {
  ChainEnd e{root, 1};
  for (int k = static_cast<int>(levels) - 1; k >= 0; --k) {
    const uint32_t nx = jump[static_cast<size_t>(k) * capacity + e.last];
    if (nx < kEnd) {
      e.last = nx;
      e.count += 1ull << k;
    }
  }
  return e;
}

// the j-th node of the chain from `root`, j below the chain's length
__device__ inline uint32_t chain_node(const uint32_t* jump, uint32_t levels, uint32_t capacity, uint32_t root,
                                      uint32_t j) {
  uint32_t node = root;
  for (uint32_t k = 0; k < levels; ++k)
    if ((j >> k) & 1u) node = jump[static_cast<size_t>(k) * capacity + node];
  return node;
}

// ---------------------------------------------------------------- reconstruction: one lane per subframe
// The lane's setup: the order bucket of the subframe that starts at bit `start` of the frame (an idle lane, bs == 0,
// has order 0).
__device__ inline int lane_bucket(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t sbps) {
  uint32_t order = 0;
  if (bs) {
    flacdec::BitReader r;
    r.init(fp, flen, start);
    flacdec::SubInfo si;
    flacdec::parse_subframe_header(r, bs, sbps, si);
    order = si.order;
  }
  return flacdec::order_bucket(order);
}

// The ladder: runs the statement given behind `bucket` once, with MAXP (a constant expression) the largest order
// bucket of the wave's lanes, so that the whole wave runs one SubDecoder<MAXP>.
#define AT_WAVE_BUCKET(bucket, ...)   \
  do {                                \
    if (__any((bucket) == 32)) {      \
      constexpr int MAXP = 32;        \
      __VA_ARGS__;                    \
    } else if (__any((bucket) == 16)) { \
      constexpr int MAXP = 16;        \
      __VA_ARGS__;                    \
    } else if (__any((bucket) == 8)) { \
      constexpr int MAXP = 8;         \
      __VA_ARGS__;                    \
    } else {                          \
      constexpr int MAXP = 4;         \
      __VA_ARGS__;                    \
    }                                 \
  } while (0)

// The wide ladder: AT_WAVE_BUCKET once more, with WIDE (a constant expression) the decoder instance and ON (a lane's
// flag) whether the lane takes part.  `deep` is the kernel's template flag: the launch may hold frames that take the
// wide decoder.  A kernel that is not deep holds the narrow instance alone, with every lane on -- the code, and the
// registers, it had before there was a wide one; a launch of shallow streams runs that kernel.  In a deep kernel `wide`
// is flacdec::needs_wide of the depth of the lane's frame; both lanes of a stereo pair hold the same frame, so they
// agree and stay together.  A wave none of whose lanes is wide runs the narrow instance with every lane on.  A wave
// with a wide lane runs the wide instance on its wide lanes and, where it also holds others, the narrow instance on
// those first -- so what a frame decodes to never depends on its neighbours in the wave, also where the two value rules
// (flac_decode_core.h) differ.  A lane that is not ON runs the statement as an idle lane does.
#define AT_WAVE_DECODER(deep, bucket, wide, ...)            \
  do {                                                      \
    if constexpr (deep) {                                   \
      if (__any(wide)) {                                    \
        if (__any(!(wide))) {                               \
          constexpr bool WIDE = false;                      \
          const bool ON = !(wide);                          \
          AT_WAVE_BUCKET(ON ? (bucket) : 4, __VA_ARGS__);   \
        }                                                   \
        constexpr bool WIDE = true;                         \
        const bool ON = (wide);                             \
        AT_WAVE_BUCKET(ON ? (bucket) : 4, __VA_ARGS__);     \
      } else {                                              \
        constexpr bool WIDE = false;                        \
        const bool ON = true;                               \
        AT_WAVE_BUCKET(bucket, __VA_ARGS__);                \
      }                                                     \
    } else {                                                \
      constexpr bool WIDE = false;                          \
      const bool ON = true;                                 \
      AT_WAVE_BUCKET(bucket, __VA_ARGS__);                  \
    }                                                       \
  } while (0)

// does a table hold a stream that takes the wide decoder?  (host: which kernel a batch call launches)
inline bool any_deep_stream(const flacenc_hip_stream_desc* d, size_t n) {
  for (size_t s = 0; s < n; ++s)
    if (flacdec::needs_wide(d[s].bits_per_sample)) return true;
  return false;
}

// The sample step of channel c: the subframe's next value, exchanged with the pair lane and stereo undone where the
// frame is a stereo pair (which sits on an even / odd lane pair; both lanes take the step together).
template <int MAXP>
__device__ __forceinline__ int32_t next_sample(flacdec::SubDecoder<MAXP>& d, uint32_t ch_tag, uint32_t c) {
  int32_t v = d.next();
  if (ch_tag >= 8) {
    const int32_t o = __shfl_xor(v, 1);
    int32_t a = c == 0 ? v : o, b = c == 0 ? o : v;
    flacdec::undo_stereo(ch_tag, a, b);
    v = c == 0 ? a : b;
  }
  return v;
}

// The same step of the wide decoder: the pair lanes exchange the full 64-bit value (two 32-bit moves), stereo is undone
// in 64 bits and the low 32 bits are the sample (flac_decode_core.h's value rule).
template <int MAXP>
__device__ __forceinline__ int32_t next_sample(flacdec::WideSubDecoder<MAXP>& d, uint32_t ch_tag, uint32_t c) {
  int64_t v = d.next();
  if (ch_tag >= 8) {
    const uint64_t u = static_cast<uint64_t>(v);
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(u), 1), hi = __shfl_xor(static_cast<uint32_t>(u >> 32), 1);
    const int64_t o = static_cast<int64_t>(static_cast<uint64_t>(hi) << 32 | lo);
    int64_t a = c == 0 ? v : o, b = c == 0 ? o : v;
    flacdec::undo_stereo_wide(ch_tag, a, b);
    v = c == 0 ? a : b;
  }
  return static_cast<int32_t>(static_cast<uint64_t>(v));
}

// Samples [skip, skip + take) of channel c of a frame of `bs` samples into packed PCM: sample t at dst + ((t - skip) *
// channels + c) * B, the low B bytes of its value, little-endian.  The recurrence runs from sample 0 and stops at
// skip + take.  Whole samples where the address allows, else bytes: a neighbouring sample's bytes are another lane's and
// are never read back.  Both lanes of a stereo pair have the same bounds, so the exchange stays convergent.  WIDE, on: the
// instance and the lane's flag (AT_WAVE_DECODER); a lane that is not on is idle.
template <int MAXP, bool WIDE>
__device__ __forceinline__ void write_pcm(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t skip, uint32_t take,
                          uint32_t sbps, uint32_t ch_tag, uint32_t c, uint32_t channels, uint32_t B, uint8_t* dst,
                          bool on) {
  if (!on) bs = skip = take = 0;
  typename flacdec::Decoder<MAXP, WIDE>::type d;
  if (bs) d.init(fp, flen, start, bs, sbps);
  uint8_t* p = dst + static_cast<size_t>(c) * B;
  const size_t step = static_cast<size_t>(channels) * B;
  const bool whole = (B == 2 || B == 4) && (reinterpret_cast<uintptr_t>(p) & (B - 1)) == 0;
  const uint32_t stop = skip + take;
  for (uint32_t t = 0; t < stop; ++t) {
    const uint32_t u = static_cast<uint32_t>(next_sample(d, ch_tag, c));
    if (t < skip) continue;
    if (whole && B == 2) {
      *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(u);
    } else if (whole) {
      *reinterpret_cast<uint32_t*>(p) = u;
    } else {
      for (uint32_t k = 0; k < B; ++k) p[k] = static_cast<uint8_t>(u >> (8u * k));
    }
    p += step;
  }
}

// The planar writer.  LDS words per lane: 16 staged elements and up to 3 carried over, padded so that the lanes' 16-byte
// reads fall on different banks (flac_decode.cpp's run_subframe stages 16 in 20 words the same way).
constexpr int kPlanarStage = 20;

// A lane's stage: stage[k] is the element that belongs at to[k], `to` 16-byte aligned; the first `lead` of the `fill`
// staged words are no elements of the lane's (they stand for the row's neighbours in front of a row that does not start
// at a 16-byte boundary) and are never stored.
struct PlanarStage {
  uint32_t* to;
  uint32_t lead, fill;
};

// Stores the whole 16-byte vectors staged -- the first one element by element where it holds a lead -- and moves the
// up to 3 elements behind them to the front of the stage.
__device__ __forceinline__ void planar_flush(PlanarStage& s, uint32_t* stage) {
  const uint32_t vectors = s.fill >> 2;
  if (vectors == 0) return;
  for (uint32_t g = 0; g < vectors; ++g) {
    if (g == 0 && s.lead) {
      for (uint32_t k = s.lead; k < 4; ++k) s.to[k] = stage[k];
    } else {
      *reinterpret_cast<uint4*>(s.to + 4 * g) = *reinterpret_cast<const uint4*>(stage + 4 * g);
    }
  }
  const uint32_t rest = s.fill & 3u;
  for (uint32_t k = 0; k < rest; ++k) stage[k] = stage[4 * vectors + k];
  s.to += 4 * vectors;
  s.lead = 0;
  s.fill = rest;
}

// Samples [skip, skip + take) of channel c of a frame of `bs` samples as 4-byte elements (streamplanar::element) to
// row[0 .. take): `row` is 4-byte aligned and nothing more, and the elements on either side of the interval are other
// lanes' (the range's neighbouring frames), so none of them is touched.  Elements are staged in `stage` (kPlanarStage
// words of LDS of the lane's own) at the place they have behind the last 16-byte boundary at or in front of them
// (streamplanar::lead), and the stage is flushed where the FRAME's sample index is 15 mod 16 -- at the same trip of
// the loop for every lane of the wave, whatever its window, so the wave runs the flush once per 16 samples -- and at the
// end: the elements up to the first boundary leave one by one (streamplanar::split's head), whole vectors as 16-byte
// stores, and what is left behind the last boundary one by one.  One loop over the recurrence, as in write_pcm: both
// lanes of a stereo pair have the same skip and take -- only their rows differ -- so the exchange stays convergent
// whatever the rows' alignment.  A float32 element of a stream of more than 24 bits is float(v), rounded to nearest
// even, times 2^-(bits - 1): it is no longer exact and can equal 1.0 (streamplanar::element).
template <int MAXP, bool WIDE>
__device__ __forceinline__ void write_planar(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t skip, uint32_t take,
                             uint32_t sbps, uint32_t ch_tag, uint32_t c, uint32_t sample_format, float scale,
                             uint32_t* row, uint32_t* stage, bool on) {
  if (!on) bs = skip = take = 0;
  typename flacdec::Decoder<MAXP, WIDE>::type d;
  if (bs) d.init(fp, flen, start, bs, sbps);
  PlanarStage s;
  s.lead = streamplanar::lead(reinterpret_cast<uintptr_t>(row));
  s.fill = s.lead;
  s.to = row - s.lead;
  const uint32_t stop = skip + take;
  for (uint32_t t = 0; t < stop; ++t) {
    const int32_t v = next_sample(d, ch_tag, c);
    if (t >= skip) stage[s.fill++] = streamplanar::element(v, sample_format, scale);  // at most 3 + 16 staged
    if ((t & 15u) == 15u) planar_flush(s, stage);
  }
  planar_flush(s, stage);
  for (uint32_t k = s.lead; k < s.fill; ++k) s.to[k] = stage[k];  // fewer than 4
}

}  // namespace flacenc_hip

#endif  // FLAC_DECODE_DEVICE_H_
