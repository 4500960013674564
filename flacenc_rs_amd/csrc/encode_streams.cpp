// encode_streams.cpp -- flacenc_hip_encode_streams: a batch of PCM streams to FLAC frames in one call, with a number of
// synchronisations and transfers that does not depend on the number of streams.
//
// The host builds the plan (stream_encode_core.h): frames sorted into classes -- (channels, bits, bytes, rate) --, inside
// a class the full blocks of every stream, then the last blocks sorted by length.  Two kernels of this file carry every
// sample and every output byte:
//   streams_fill_kernel   FrameBuf::fill_le_bytes for a table of frames taken from many streams: from any byte offset
//                         into 16-byte aligned channel-major int32 rows, zero beyond the frame's samples
//   streams_place_kernel  a frame packed with number 0, from its pack slot at its launch position into its stream's slot
//                         with its index in the stream as the frame number: new header, new CRC-8, the CRC-16 combined
//                         from the old one, the body moved with destination-aligned dwords
// Between them the existing frame-level calls run unchanged, once per run of the plan, with first_frame_number = 0 and
// frame_number_step = 0.  Lengths, offsets and the cut per stream are three small launches (the scan is
// stream_index.cpp's, the cut streambatch::accepted_frames).
#include "api_internal.h"
#include "stream_batch_core.h"
#include "stream_encode_core.h"
#include "stream_index.h"
#include "stream_planar_encode_core.h"

namespace flacenc_hip {
namespace {

using streamenc::LaunchFrame;
using streamenc::StreamFrame;
using Desc = flacenc_hip_pcm_stream_desc;

static_assert(sizeof(Desc) == 48 && sizeof(LaunchFrame) == 16 && sizeof(StreamFrame) == 24, "table layouts");

__constant__ vbs::XPow8 kXPow8 = vbs::make_xpow8();

enum : uint32_t { M_FRAMES = 0, M_BYTES = 1, M_WORDS = 8 };  // meta (uint64): what the call adds up

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

// ---------------------------------------------------------------- fill
// The aligned dword at p, of which only the bytes inside [lo, hi) are read; the others are zero.
__device__ inline uint32_t load_inside(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (p + b >= lo && p + b < hi) v |= static_cast<uint32_t>(p[b]) << (8 * b);
  return v;
}

// the little-endian, sign-extended sample of B bytes at byte `o` of the dwords d[]
template <int B>
__device__ inline int32_t sample_at(const uint32_t* d, int o) {
  const int i = o >> 2, s = o & 3;
  uint32_t u = d[i] >> (8 * s);
  if (s + B > 4) u |= d[i + 1] << (32 - 8 * s);
  return static_cast<int32_t>(u << (32 - 8 * B)) >> (32 - 8 * B);
}

// One lane: four sample times of one frame, all channels.  Its source is C*B dwords' worth of bytes at an arbitrary byte
// offset: C*B + 1 aligned loads, shifted into place with v_alignbyte_b32; its output one 16-byte store per channel.  The
// work items (frame, group of four sample times) are numbered flat and walked grid-stride, so neither the frames nor the
// block size are bounded by a grid dimension.  Rows are `groups` * 4 = stride words long: what lies beyond the frame's
// valid samples is written as zero (a tail frame's row is zero up to the full stride).  No byte outside the frame's span
// [pcm_offset, pcm_offset + valid*C*B) is read: the first and last dword of a frame go through load_inside.
template <int C, int B>
__global__ void __launch_bounds__(256) streams_fill_kernel(const uint8_t* __restrict__ pcm,
                                                           const LaunchFrame* __restrict__ table, uint32_t n_frames,
                                                           uint32_t row0, uint32_t groups, size_t stride,
                                                           int32_t* __restrict__ rows) {
  constexpr int ND = C * B;
  const uint64_t items = static_cast<uint64_t>(n_frames) * groups;
  const bool narrow = items <= 0xFFFFFFFFull;
  for (uint64_t it = blockIdx.x * 256ull + threadIdx.x; it < items; it += static_cast<uint64_t>(gridDim.x) * 256ull) {
    const uint32_t f = narrow ? static_cast<uint32_t>(it) / groups : static_cast<uint32_t>(it / groups);
    const uint32_t t0 = static_cast<uint32_t>(it - static_cast<uint64_t>(f) * groups) * 4u;
    const LaunchFrame fr = table[f];
    uint32_t d[ND + 1];
#pragma unroll
    for (int j = 0; j <= ND; ++j) d[j] = 0;
    if (t0 < fr.valid) {
      const uint8_t* lo = pcm + fr.pcm_offset;
      const uint8_t* hi = lo + static_cast<size_t>(fr.valid) * (C * B);
      const uint8_t* a = lo + static_cast<size_t>(t0) * (C * B);
      const uint32_t skew = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a)) & 3u;
      const uint8_t* base = a - skew;
      uint32_t w[ND + 1];
      if (base >= lo && base + 4 * (ND + 1) <= hi) {
#pragma unroll
        for (int j = 0; j <= ND; ++j) w[j] = reinterpret_cast<const uint32_t*>(base)[j];
      } else {
#pragma unroll
        for (int j = 0; j <= ND; ++j) w[j] = load_inside(base + 4 * j, lo, hi);
      }
#pragma unroll
      for (int j = 0; j < ND; ++j) d[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], skew);
    }
    int32_t* dst = rows + (static_cast<size_t>(row0) + f) * C * stride + t0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      int4 v;
      v.x = sample_at<B>(d, (0 * C + c) * B);
      v.y = sample_at<B>(d, (1 * C + c) * B);
      v.z = sample_at<B>(d, (2 * C + c) * B);
      v.w = sample_at<B>(d, (3 * C + c) * B);
      *reinterpret_cast<int4*>(dst + static_cast<size_t>(c) * stride) = v;
    }
  }
}

template <int C>
hipError_t launch_fill_c(uint32_t B, dim3 grid, hipStream_t st, const uint8_t* pcm, const LaunchFrame* table,
                         uint32_t n_frames, uint32_t row0, uint32_t groups, size_t stride, int32_t* rows) {
  switch (B) {
    case 1: hipLaunchKernelGGL((streams_fill_kernel<C, 1>), grid, dim3(256), 0, st, pcm, table, n_frames, row0, groups, stride, rows); break;
    case 2: hipLaunchKernelGGL((streams_fill_kernel<C, 2>), grid, dim3(256), 0, st, pcm, table, n_frames, row0, groups, stride, rows); break;
    case 3: hipLaunchKernelGGL((streams_fill_kernel<C, 3>), grid, dim3(256), 0, st, pcm, table, n_frames, row0, groups, stride, rows); break;
    default: hipLaunchKernelGGL((streams_fill_kernel<C, 4>), grid, dim3(256), 0, st, pcm, table, n_frames, row0, groups, stride, rows); break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------- lengths and the cut
// stream position q: the frame's length with its own number, as a scan input and as the caller's frame_lengths entry
__global__ void __launch_bounds__(256) streams_newlen_kernel(const StreamFrame* __restrict__ sf,
                                                             const uint32_t* __restrict__ len0, uint32_t n_frames,
                                                             uint64_t* __restrict__ newlen,
                                                             uint32_t* __restrict__ frame_lengths) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_frames) return;
  const uint32_t l = streamenc::renumbered_length(len0[sf[q].launch_pos], sf[q].index);
  newlen[q] = l;
  frame_lengths[q] = l;
}

// one lane per stream: the longest prefix of whole frames that fits the slot, the stream's totals, the call's sums
__global__ void __launch_bounds__(256) streams_cut_kernel(const Desc* __restrict__ descs,
                                                          const uint32_t* __restrict__ first, uint32_t n_streams,
                                                          const uint64_t* __restrict__ off,
                                                          const uint64_t* __restrict__ zeros,
                                                          uint32_t* __restrict__ s_accepted, uint64_t* __restrict__ s_bytes,
                                                          uint64_t* __restrict__ totals, uint64_t* __restrict__ meta) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  const uint64_t q0 = first[s], count = first[s + 1] - q0;
  const uint64_t frames = streambatch::accepted_frames(off, zeros, q0, count, descs[s].out_capacity);
  const uint64_t bytes = off[q0 + frames] - off[q0];
  s_accepted[s] = static_cast<uint32_t>(frames);
  s_bytes[s] = bytes;
  totals[4 * static_cast<size_t>(s) + 0] = frames;
  totals[4 * static_cast<size_t>(s) + 1] = bytes;
  totals[4 * static_cast<size_t>(s) + 2] = q0;
  totals[4 * static_cast<size_t>(s) + 3] = frames < count ? FLACENC_HIP_ENCODE_NO_ROOM : 0u;
  if (frames) {
    atomicAdd(reinterpret_cast<unsigned long long*>(meta + M_FRAMES), static_cast<unsigned long long>(frames));
    atomicAdd(reinterpret_cast<unsigned long long*>(meta + M_BYTES), static_cast<unsigned long long>(bytes));
  }
}

// ---------------------------------------------------------------- place
// A workgroup per frame in stream order (grid-stride).  The body moves as place_frames_kernel moves frames; wave 0
// writes the renumbered header and the CRC-16 as rehead_kernel does: x^(8|B|) is the product of the XPOW8 entries of
// |B|'s set bits, one per lane, reduced across the wave, so the body is not read a second time.  A frame behind its
// stream's cut is not written.  A stream's frames start at out + where[stream] (`where` given: the compact staging of
// the host path) or at out + its out_offset.
__global__ void __launch_bounds__(256) streams_place_kernel(const uint8_t* __restrict__ pack,
                                                            const StreamFrame* __restrict__ sf,
                                                            const uint32_t* __restrict__ len0, uint32_t n_frames,
                                                            const Desc* __restrict__ descs,
                                                            const uint32_t* __restrict__ first,
                                                            const uint32_t* __restrict__ s_accepted,
                                                            const uint64_t* __restrict__ off,
                                                            const uint64_t* __restrict__ where, uint8_t* __restrict__ out) {
  for (uint32_t q = blockIdx.x; q < n_frames; q += gridDim.x) {
    const StreamFrame fr = sf[q];
    if (fr.index >= s_accepted[fr.stream]) continue;
    const uint8_t* src = pack + fr.pack_offset;
    const uint32_t flen = len0[fr.launch_pos];
    const uint32_t hf = vbs::header_bytes(src);
    // (the frame must take exactly the bytes the scan gave it: a header that disagrees is not written at all)
    if (hf == 0 || flen < hf + 2u || flen > fr.pack_room) continue;
    const uint32_t hv = streamenc::renumbered_header_bytes(src, fr.index);
    if (flen - hf + hv != streamenc::renumbered_length(flen, fr.index)) continue;
    uint8_t* dst = out + (where ? where[fr.stream] : descs[fr.stream].out_offset) + (off[q] - off[first[fr.stream]]);
    const uint32_t body = flen - 2u - hf;
    {
      const uint8_t* s = src + hf;
      uint8_t* d = dst + hv;
      uint32_t len = body;
      uint32_t head = static_cast<uint32_t>(-reinterpret_cast<uintptr_t>(d)) & 3u;
      if (head > len) head = len;
      if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
      s += head;
      d += head;
      len -= head;
      const uint32_t n_dwords = len >> 2;
      const uint32_t skew = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s)) & 3u;
      const uint32_t* sw = reinterpret_cast<const uint32_t*>(s - skew);
      uint32_t* dw = reinterpret_cast<uint32_t*>(d);
      if (skew == 0) {
        for (uint32_t k = threadIdx.x; k < n_dwords; k += blockDim.x) dw[k] = sw[k];
      } else {
        // (the last aligned source dword lies inside the 16-byte aligned pack slot: the CRC-16 bytes follow the body)
        for (uint32_t k = threadIdx.x; k < n_dwords; k += blockDim.x) dw[k] = __builtin_amdgcn_alignbyte(sw[k + 1], sw[k], skew);
      }
      const uint32_t tail = len & 3u;
      if (threadIdx.x < tail) d[n_dwords * 4 + threadIdx.x] = s[n_dwords * 4 + threadIdx.x];
    }
    if (threadIdx.x < 64) {
      const uint32_t lane = threadIdx.x;
      uint32_t p = (lane < 32 && ((body >> lane) & 1u)) ? kXPow8.v[lane] : 1u;
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) p = flacdec::crc16_mulmod(p, __shfl_xor(p, m, 64));
      if (lane == 0) {
        uint8_t hd[16];
        streamenc::write_renumbered_header(src, fr.index, hd);
        for (uint32_t k = 0; k < hv; ++k) dst[k] = hd[k];
        const uint32_t crc_old = (static_cast<uint32_t>(src[flen - 2]) << 8) | src[flen - 1];
        const uint32_t crc = vbs::crc16_combine(crc_old, vbs::crc16_bytes(src, hf), vbs::crc16_bytes(hd, hv), p);
        dst[hv + body] = static_cast<uint8_t>(crc >> 8);
        dst[hv + body + 1] = static_cast<uint8_t>(crc);
      }
    }
  }
}

// the handle's stream is drained before an error hands the handle back
struct Drain {
  flacenc_hip_handle* h;
  bool armed = true;
  ~Drain() {
    if (armed) (void)hipStreamSynchronize(h->stream);
  }
};

}  // namespace

hipError_t launch_streams_fill(const uint8_t* pcm, const LaunchFrame* table, uint32_t n_frames, uint32_t channels,
                               uint32_t bytes_per_sample, uint32_t row0, size_t stride, int32_t* rows,
                               hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  const uint32_t groups = static_cast<uint32_t>(stride / 4);
  const uint64_t items = static_cast<uint64_t>(n_frames) * groups;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((items + 255) / 256, 65536)));
  const uint32_t B = bytes_per_sample;
#define ES_FILL(C) \
  case C: return launch_fill_c<C>(B, grid, stream, pcm, table, n_frames, row0, groups, stride, rows)
  switch (channels) {
    ES_FILL(1);
    ES_FILL(2);
    ES_FILL(3);
    ES_FILL(4);
    ES_FILL(5);
    ES_FILL(6);
    ES_FILL(7);
    ES_FILL(8);
  }
#undef ES_FILL
  return hipErrorInvalidValue;
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" size_t flacenc_hip_encode_streams_frames(const void* streams, size_t n_streams, uint32_t block_size) {
  const uint64_t n = streamenc::count_frames(static_cast<const Desc*>(streams), n_streams, block_size);
  return n > static_cast<uint64_t>(SIZE_MAX) ? SIZE_MAX : static_cast<size_t>(n);
}

extern "C" int flacenc_hip_encode_streams(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                                          uint64_t pcm_bytes, const void* streams, size_t n_streams, uint32_t block_size,
                                          uint8_t* out, uint64_t out_bytes, uint32_t* frame_lengths, size_t max_frames,
                                          uint64_t* totals, uint64_t call_totals[2], int memory_kind) {
  return encode_streams_common(h, cfg, pcm, pcm_bytes, nullptr, streams, n_streams, block_size, out, out_bytes,
                               frame_lengths, max_frames, totals, call_totals, memory_kind);
}

// Both entry points.  `planar` null: the packed PCM of flacenc_hip_encode_streams.  Else pcm is null and the samples are
// the rows `planar` describes; everything behind the fill -- plan, scratch, runs, scan, cut, place, host staging -- is
// the same code, and the digests and clip counts ride in the result transfer that is there anyway.
int flacenc_hip::encode_streams_common(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                                       uint64_t pcm_bytes, const PlanarSource* planar, const void* streams,
                                       size_t n_streams, uint32_t block_size, uint8_t* out, uint64_t out_bytes,
                                       uint32_t* frame_lengths, size_t max_frames, uint64_t* totals,
                                       uint64_t call_totals[2], int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  // [0] launches of this file's kernels (and, planar, of encode_streams_planar.cpp's and the digests'), [1] host
  // synchronisations, [2] host-device transfers, [3] classes, [4] full-frame runs, [5] tail runs, [6] frame-level calls
  // (= [4] + [5]), [7] the launches among [0] that the digests cost (0 for flacenc_hip_encode_streams)
  uint64_t* plan = h->last_encode_streams_plan;
  for (int i = 0; i < 8; ++i) plan[i] = 0;
  const void* input = planar ? planar->samples : pcm;
  if ((memory_kind != FLACENC_HIP_MEM_HOST && memory_kind != FLACENC_HIP_MEM_DEVICE) || !cfg || !input || !streams || !out ||
      !frame_lengths || !totals || !call_totals || n_streams > streamenc::MAX_STREAMS) {
    h->last_error = planar ? "encode_streams_planar: null pointer, unknown memory kind or more than 2^24 streams"
                           : "encode_streams: null pointer, unknown memory kind or more than 2^24 streams";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const Desc* table = static_cast<const Desc*>(streams);
  if (planar) {
    // the rows against `samples`; a device pointer must be aligned as its elements are
    if (planarenc::check_rows(table, n_streams, planar->sample_format, planar->row_pitch, planar->samples_bytes) !=
            FLACENC_HIP_OK ||
        (memory_kind == FLACENC_HIP_MEM_DEVICE && (reinterpret_cast<uintptr_t>(planar->samples) & 3u))) {
      h->last_error = "encode_streams_planar: unknown sample_format, an offset that is no multiple of 4, a row_pitch below "
                      "a stream's total_samples, rows past samples_bytes, or device samples not 4-byte aligned";
      return FLACENC_HIP_ERR_BAD_ARGUMENT;
    }
  }
  const uint32_t max_bits = h->max_encode_bps;
  int rc = streamenc::check_streams(table, planar ? 0 : n_streams, pcm_bytes, out_bytes, block_size, max_bits);
  for (size_t s = 0; planar && rc == FLACENC_HIP_OK && s < n_streams; ++s) {
    // the packed PCM exists nowhere: every other rule holds, the span is held against a buffer without end
    Desc x = table[s];
    x.offset = 0;
    if (x.total_samples >= (streamenc::MAX_FRAMES << 15)) rc = FLACENC_HIP_ERR_BAD_ARGUMENT;  // 2^31 frames at any block size
    // (a float32 element holds 24 bits: deeper streams come as int32 alone)
    if (is_wide(x.bits_per_sample) && planar->sample_format != FLACENC_HIP_SAMPLE_I32) rc = FLACENC_HIP_ERR_BAD_ARGUMENT;
    if (rc == FLACENC_HIP_OK) rc = streamenc::check_streams(&x, 1, UINT64_MAX, out_bytes, block_size, max_bits);
  }
  const uint64_t F64 = rc == FLACENC_HIP_OK ? streamenc::count_frames(table, n_streams, block_size) : 0;
  if (rc != FLACENC_HIP_OK || F64 >= streamenc::MAX_FRAMES || F64 > max_frames) {
    h->last_error = "encode_streams: block_size not in 64..=32767, channels not in 1..=8, bytes_per_sample not in 1..=4, "
                    "bits_per_sample not in 8..=24 (..=32 at 4 bytes after flacenc_hip_set_max_encode_bits_per_sample; int32 "
                    "elements only), a span past pcm_bytes, a slot past out_bytes, 2^31 frames or more, or "
                    "max_frames below flacenc_hip_encode_streams_frames";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if ((rc = flacenc_hip_verify_config(&cfg->qlpc)) != FLACENC_HIP_OK) return rc;
  call_totals[0] = call_totals[1] = 0;
  if (n_streams == 0) return FLACENC_HIP_OK;
  const bool host = memory_kind == FLACENC_HIP_MEM_HOST;
  const uint32_t ns = static_cast<uint32_t>(n_streams), F = static_cast<uint32_t>(F64);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;

  // ---- the plan ----
  const size_t override_chunk = h->encode_streams_chunk_override;
  streamenc::Plan pl;
  try {
    pl = streamenc::build_plan(
        table, n_streams, block_size,
        [&](const streamenc::Class& k) -> uint32_t {
          // as flacenc_hip_encode_pcm's chunk: enough frames to fill the device, few enough to bound the candidates' scratch
          if (override_chunk) return static_cast<uint32_t>(override_chunk);
          const size_t frame_in_bytes = static_cast<size_t>(block_size) * k.channels * k.bytes_per_sample;
          const size_t c = (48u << 20) / frame_in_bytes;
          return static_cast<uint32_t>(c < 768 ? 768 : (c > 8192 ? 8192 : c));
        },
        [](uint32_t channels, uint32_t n, uint32_t bits) -> size_t {
          return channels == 2 ? flacenc_hip_stereo_frame_bytes_bound(n, bits) : flacenc_hip_frame_bytes_bound(channels, n, bits);
        });
  } catch (...) {
    h->last_error = "encode_streams: out of host memory";
    return FLACENC_HIP_ERR_DEVICE;
  }
  plan[3] = pl.classes.size();
  plan[4] = pl.full_runs;
  plan[5] = pl.tail_runs;
  plan[6] = pl.runs.size();

  // ---- pinned staging of the tables; the results come down into the other slot ----
  const size_t o_tdesc = 0, o_tfirst = a256(o_tdesc + n_streams * sizeof(Desc));
  const size_t o_tlaunch = a256(o_tfirst + (n_streams + 1) * 4), o_tstream = a256(o_tlaunch + static_cast<size_t>(F) * sizeof(LaunchFrame));
  // planar: its frames in launch order in place of the LaunchFrames, its streams, the lengths of their packed PCM
  const size_t o_tpframe = a256(o_tstream + static_cast<size_t>(F) * sizeof(StreamFrame));
  const size_t o_tpstream = a256(o_tpframe + (planar ? static_cast<size_t>(F) * sizeof(planarenc::Frame) : 0));
  const size_t o_tplen = a256(o_tpstream + (planar ? n_streams * sizeof(planarenc::Stream) : 0));
  const size_t table_bytes = a256(o_tplen + (planar ? n_streams * 8 : 0));
  // results, one transfer: meta | totals | where | (planar: digests | clip counts) | frame lengths (host memory; device
  // memory: meta alone)
  const size_t w_digests = M_WORDS + 4 * n_streams + (n_streams + 1), w_clipped = w_digests + (planar ? 2 * n_streams : 0);
  const size_t result_words = w_clipped + (planar ? n_streams : 0);
  const size_t result_bytes = result_words * 8 + static_cast<size_t>(F) * 4;
  if ((rc = ensure_pinned(h, h->pin_meta, &h->pin_meta_cap, table_bytes > result_bytes ? table_bytes : result_bytes)) !=
      FLACENC_HIP_OK)
    return rc;
  char* p_table = static_cast<char*>(h->pin_meta[1]);
  std::memcpy(p_table + o_tdesc, table, n_streams * sizeof(Desc));
  std::memcpy(p_table + o_tfirst, pl.stream_first.data(), (n_streams + 1) * 4);
  if (F) {
    if (!planar) std::memcpy(p_table + o_tlaunch, pl.launch.data(), static_cast<size_t>(F) * sizeof(LaunchFrame));
    std::memcpy(p_table + o_tstream, pl.stream.data(), static_cast<size_t>(F) * sizeof(StreamFrame));
  }
  // planar: elements are counted from the first byte that holds one (host memory: only those bytes go up)
  const bool want_digests = planar && planar->digests, want_clipped = planar && planar->clipped;
  planarenc::Extent ext = {0, 0};
  uint64_t image_bytes = 0;
  uint32_t pack_per = 0;  // the most dwords of packed PCM a frame of the table starts
  if (planar) {
    if (host) ext = planarenc::extent(table, n_streams, planar->row_pitch);
    planarenc::Stream* ps = reinterpret_cast<planarenc::Stream*>(p_table + o_tpstream);
    uint64_t* plen = reinterpret_cast<uint64_t*>(p_table + o_tplen);
    for (size_t s = 0; s < n_streams; ++s) {
      const Desc& d = table[s];
      plen[s] = planarenc::packed_bytes(d.total_samples, d.channels, d.bytes_per_sample);
      ps[s] = {d.total_samples ? (d.offset - ext.first) / 4 : 0, planarenc::pitch_of(planar->row_pitch, d.total_samples),
               image_bytes, d.total_samples};
      if (want_digests) image_bytes += planarenc::packed_room(plen[s]);
      const uint32_t per = static_cast<uint32_t>((static_cast<uint64_t>(block_size) * d.channels * d.bytes_per_sample + 3) / 4);
      if (per > pack_per) pack_per = per;
    }
    planarenc::Frame* pf = reinterpret_cast<planarenc::Frame*>(p_table + o_tpframe);
    for (uint32_t p = 0; p < F; ++p) {
      const StreamFrame& q = pl.stream[pl.launch[p].stream_pos];
      const uint64_t t = static_cast<uint64_t>(q.index) * block_size;
      pf[p] = {ps[q.stream].elem0 + t, ps[q.stream].pitch, pl.launch[p].valid, q.stream, t};
    }
  }

  // ---- device scratch: everything is sized before anything is enqueued (ensure does not keep contents) ----
  size_t need = 0;
  auto take = [&need](size_t bytes_) {
    const size_t at = need;
    need += a256(bytes_ + 8);
    return at;
  };
  const size_t o_result = take(result_bytes), o_table = take(table_bytes);
  const size_t o_sbytes = take(n_streams * 8), o_sacc = take(n_streams * 4);
  const size_t o_len0 = take(static_cast<size_t>(F) * 4), o_newlen = take(static_cast<size_t>(F) * 8);
  const size_t o_off = take((static_cast<size_t>(F) + 1) * 8), o_zeros = take((static_cast<size_t>(F) + 1) * 8);
  if ((rc = ensure(h, h->d_encs, need)) != FLACENC_HIP_OK) return rc;
  const size_t stride = padded_stride(block_size);
  size_t max_run = 1, max_record = sizeof(flacenc_hip_stereo_frame_result), max_wide = 0;
  for (const streamenc::Run& r : pl.runs) {
    const streamenc::Class& k = pl.classes[r.cls];
    if (is_wide(k.bits_per_sample)) {  // the wide step's records, sized here so that no run allocates
      const size_t recs = r.frames * wideenc::roles_of(k.channels) * sizeof(wideenc::SubRecord);
      if (recs > max_wide) max_wide = recs;
      continue;
    }
    const size_t rec = r.frames * (k.channels == 2 ? sizeof(flacenc_hip_stereo_frame_result)
                                                   : k.channels * sizeof(flacenc_hip_channel_result));
    if (rec > max_record) max_record = rec;
    if (r.frames > max_run) max_run = r.frames;
  }
  if ((rc = ensure(h, h->d_samples, static_cast<size_t>(pl.max_class_rows) * stride * 4 + 16)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_results, max_record)) != FLACENC_HIP_OK) return rc;
  if (max_wide && (rc = ensure(h, h->d_wide, max_wide)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_pack[0], static_cast<size_t>(pl.pack_bytes) + 16)) != FLACENC_HIP_OK) return rc;
  const uint8_t* d_pcm = planar ? static_cast<const uint8_t*>(planar->samples) : pcm;
  if (planar) pcm_bytes = ext.end - ext.first;  // what a host call sends up
  if (want_digests && (rc = ensure(h, h->d_pcm[1], static_cast<size_t>(image_bytes) + 16)) != FLACENC_HIP_OK) return rc;
  if (host) {
    if ((rc = ensure(h, h->d_pcm[0], static_cast<size_t>(pcm_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_pcm = static_cast<const uint8_t*>(h->d_pcm[0].ptr);
    if ((rc = ensure_copy_pool(h, "encode_streams")) != FLACENC_HIP_OK) return rc;
  }
  char* S = static_cast<char*>(h->d_encs.ptr);
  uint64_t* meta = reinterpret_cast<uint64_t*>(S + o_result);
  uint64_t* d_totals = host ? meta + M_WORDS : totals;
  uint64_t* where = host ? meta + M_WORDS + 4 * n_streams : nullptr;
  uint32_t* d_flen = host ? reinterpret_cast<uint32_t*>(meta + result_words) : frame_lengths;
  uint8_t* d_digests = !want_digests ? nullptr : host ? reinterpret_cast<uint8_t*>(meta + w_digests) : planar->digests;
  unsigned long long* d_clipped =
      reinterpret_cast<unsigned long long*>(!want_clipped ? nullptr : host ? meta + w_clipped : planar->clipped);
  const uint32_t* elems = reinterpret_cast<const uint32_t*>(d_pcm);
  const planarenc::Frame* t_pframe = reinterpret_cast<const planarenc::Frame*>(S + o_table + o_tpframe);
  const planarenc::Stream* t_pstream = reinterpret_cast<const planarenc::Stream*>(S + o_table + o_tpstream);
  const uint64_t* t_plen = reinterpret_cast<const uint64_t*>(S + o_table + o_tplen);
  const Desc* descs = reinterpret_cast<const Desc*>(S + o_table + o_tdesc);
  const uint32_t* first = reinterpret_cast<const uint32_t*>(S + o_table + o_tfirst);
  const LaunchFrame* t_launch = reinterpret_cast<const LaunchFrame*>(S + o_table + o_tlaunch);
  const StreamFrame* t_stream = reinterpret_cast<const StreamFrame*>(S + o_table + o_tstream);
  uint64_t* s_bytes = reinterpret_cast<uint64_t*>(S + o_sbytes);
  uint32_t* s_accepted = reinterpret_cast<uint32_t*>(S + o_sacc);
  uint32_t* len0 = reinterpret_cast<uint32_t*>(S + o_len0);
  uint64_t* newlen = reinterpret_cast<uint64_t*>(S + o_newlen);
  uint64_t* off = reinterpret_cast<uint64_t*>(S + o_off);
  uint64_t* zeros = reinterpret_cast<uint64_t*>(S + o_zeros);
  int32_t* rows = static_cast<int32_t*>(h->d_samples.ptr);
  uint8_t* pack = static_cast<uint8_t*>(h->d_pack[0].ptr);

  Drain drain{h};
  // ---- up: the tables, the PCM ----
  HIP_TRY(h, hipMemsetAsync(meta, 0, M_WORDS * 8, st));
  HIP_TRY(h, hipMemsetAsync(zeros, 0, (static_cast<size_t>(F) + 1) * 8, st));
  HIP_TRY(h, hipMemcpyAsync(S + o_table, p_table, table_bytes, hipMemcpyHostToDevice, st));
  ++plan[2];
  if (d_clipped) HIP_TRY(h, hipMemsetAsync(d_clipped, 0, n_streams * 8, st));
  if (host && pcm_bytes) {
    if (planar) pcm = static_cast<const uint8_t*>(planar->samples) + ext.first;
    const void* src = pcm;
    if (!is_pinned(pcm)) {  // pageable: through pinned staging on the handle's host threads
      if ((rc = ensure_pinned(h, h->pin_in, &h->pin_in_cap, static_cast<size_t>(pcm_bytes))) != FLACENC_HIP_OK) return rc;
      h->copy_pool->copy(h->pin_in[0], pcm, static_cast<size_t>(pcm_bytes));
      src = h->pin_in[0];
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_pcm[0].ptr, src, static_cast<size_t>(pcm_bytes), hipMemcpyHostToDevice, st));
    ++plan[2];
  }

  // ---- class after class: fill its rows (full frames, then all tails), then its runs ----
  size_t next_run = 0;
  for (size_t c = 0; c < pl.classes.size(); ++c) {
    const streamenc::Class& k = pl.classes[c];
    if (k.full) {
      if (planar)
        HIP_TRY(h, launch_planar_fill(elems, t_pframe + k.first, k.full, k.channels, planar->sample_format, k.bits_per_sample,
                                      0, stride, rows, d_clipped, h->planar_fill_form, st));
      else
        HIP_TRY(h, launch_streams_fill(d_pcm, t_launch + k.first, k.full, k.channels, k.bytes_per_sample, 0, stride, rows, st));
      ++plan[0];
    }
    if (k.tails) {
      if (planar)
        HIP_TRY(h, launch_planar_fill(elems, t_pframe + k.first + k.full, k.tails, k.channels, planar->sample_format,
                                      k.bits_per_sample, k.full, stride, rows, d_clipped, h->planar_fill_form, st));
      else
        HIP_TRY(h, launch_streams_fill(d_pcm, t_launch + k.first + k.full, k.tails, k.channels, k.bytes_per_sample, k.full,
                                       stride, rows, st));
      ++plan[0];
    }
    for (; next_run < pl.runs.size() && pl.runs[next_run].cls == c; ++next_run) {
      const streamenc::Run& r = pl.runs[next_run];
      const int32_t* run_rows = rows + static_cast<size_t>(r.first - k.first) * k.channels * stride;
      uint8_t* run_pack = pack + k.pack_base + static_cast<size_t>(r.first - k.first) * k.pack_stride;
      if (is_wide(k.bits_per_sample)) {  // the wide step in place of the frame-level calls
        rc = encode_pack_frames_wide(h, cfg, run_rows, r.frames, k.channels, r.block, stride,
                                                       k.bits_per_sample, k.sample_rate, 0, 0, run_pack, k.pack_stride,
                                                       len0 + r.first, st);
      } else if (k.channels == 2) {
        rc = flacenc_hip_encode_pack_stereo_frames_async(
            h, cfg, run_rows, r.frames, r.block, stride, k.bits_per_sample, k.sample_rate, 0, 0,
            static_cast<flacenc_hip_stereo_frame_result*>(h->d_results.ptr), run_pack, k.pack_stride, len0 + r.first, st);
      } else {
        rc = flacenc_hip_encode_pack_frames_async(
            h, cfg, run_rows, r.frames, k.channels, r.block, stride, k.bits_per_sample, k.sample_rate, 0, 0,
            static_cast<flacenc_hip_channel_result*>(h->d_results.ptr), run_pack, k.pack_stride, len0 + r.first, st);
      }
      if (rc != FLACENC_HIP_OK) return rc;
    }
  }

  // ---- planar: the packed PCM of every stream, written once for the digests, and the digests ----
  if (want_digests) {
    uint8_t* image = static_cast<uint8_t*>(h->d_pcm[1].ptr);
    if (F) {
      HIP_TRY(h, launch_planar_pack(elems, t_pframe, F, t_pstream, descs, pack_per, planar->sample_format, image, st));
      ++plan[0];
      ++plan[7];
    }
    HIP_TRY(h, launch_md5_spans(image, &t_pstream->packed_base, static_cast<uint32_t>(sizeof(planarenc::Stream) / 8), t_plen,
                                nullptr, ns, d_digests, st));
    ++plan[0];
    ++plan[7];
  }

  // ---- lengths, offsets in stream order, the cut ----
  if (F) {
    hipLaunchKernelGGL(streams_newlen_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, st, t_stream, len0, F, newlen, d_flen);
    ++plan[0];
  }
  HIP_TRY(h, streamindex::launch_scan2(newlen, nullptr, F, off, nullptr, st));
  ++plan[0];
  hipLaunchKernelGGL(streams_cut_kernel, dim3(ceil_div(ns, 256)), dim3(256), 0, st, descs, first, ns, off, zeros,
                     s_accepted, s_bytes, d_totals, meta);
  ++plan[0];
  HIP_TRY(h, hipGetLastError());
  uint8_t* d_out = out;
  const uint64_t* r_meta = static_cast<const uint64_t*>(h->pin_meta[0]);
  uint64_t out_total = 0;
  if (host) {
    // the one thing the host must wait for: how many bytes the accepted frames take, laid back to back
    HIP_TRY(h, streamindex::launch_scan2(s_bytes, nullptr, ns, where, nullptr, st));
    ++plan[0];
    HIP_TRY(h, hipMemcpyAsync(h->pin_meta[0], meta, result_bytes, hipMemcpyDeviceToHost, st));
    ++plan[2];
    HIP_TRY(h, hipStreamSynchronize(st));
    ++plan[1];
    out_total = r_meta[M_WORDS + 4 * n_streams + n_streams];
    if ((rc = ensure(h, h->d_cont[0], static_cast<size_t>(out_total) + 16)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure_pinned(h, h->pin_out, &h->pin_out_cap, static_cast<size_t>(out_total))) != FLACENC_HIP_OK) return rc;
    d_out = static_cast<uint8_t*>(h->d_cont[0].ptr);
  }

  // ---- every accepted frame to its place, with its number ----
  if (F) {
    hipLaunchKernelGGL(streams_place_kernel, dim3(F < 65536u ? F : 65536u), dim3(256), 0, st, pack, t_stream, len0, F, descs,
                       first, s_accepted, off, where, d_out);
    ++plan[0];
  }
  HIP_TRY(h, hipGetLastError());
  if (host) {
    if (out_total) {
      HIP_TRY(h, hipMemcpyAsync(h->pin_out[0], d_out, static_cast<size_t>(out_total), hipMemcpyDeviceToHost, st));
      ++plan[2];
    }
  } else {
    HIP_TRY(h, hipMemcpyAsync(h->pin_meta[0], meta, M_WORDS * 8, hipMemcpyDeviceToHost, st));
    ++plan[2];
  }
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  drain.armed = false;
  if (host) {
    const uint64_t* r_totals = r_meta + M_WORDS;
    const uint64_t* r_where = r_totals + 4 * n_streams;
    const uint8_t* staged = static_cast<const uint8_t*>(h->pin_out[0]);
    for (size_t s = 0; s < n_streams; ++s) {
      const uint64_t n = r_where[s + 1] - r_where[s];
      if (n) h->copy_pool->copy(out + table[s].out_offset, staged + r_where[s], static_cast<size_t>(n));
    }
    std::memcpy(totals, r_totals, n_streams * 32);
    if (want_digests) std::memcpy(planar->digests, r_meta + w_digests, n_streams * 16);
    if (want_clipped) std::memcpy(planar->clipped, r_meta + w_clipped, n_streams * 8);
    if (F) std::memcpy(frame_lengths, r_meta + result_words, static_cast<size_t>(F) * 4);
  }
  call_totals[0] = r_meta[M_FRAMES];
  call_totals[1] = r_meta[M_BYTES];
  return FLACENC_HIP_OK;
}
