// flac_recover_streams.cpp -- flacenc_hip_recover_streams: a batch of damaged FLAC streams decoded through their errors
// in one call, with a number of launches, synchronisations and transfers that depends neither on the number of streams
// nor on the damage.  The rule is stated at the call in include/flacenc_hip.h.
//
// The index is streamindex::build in its resynchronising form (Request::resync, stream_index.h): every stream's chain
// runs over the verified candidates of its span, whatever lies between them, every chain frame is enumerated in `slot`
// order and every candidate's coded number is kept.  This file holds what follows it, over that frame sequence
// (stream_recover_core.h holds the arithmetic):
//   recover_position_kernel   a frame's coded position P, what it adds to the prefix maximum, and -- by atomics per
//                             stream -- the bytes the chain covers and its inner breaks
//   segmax_*_kernel           the segmented inclusive max-scan of the frames' ends per stream: a workgroup's aggregate,
//                             one workgroup over the aggregates, the aggregates applied.  Three launches for any number
//                             of frames and streams
//   recover_place_kernel      the placement flag; its scan and recover_list_kernel give the list of placed frames
//   recover_cut_kernel        one lane per stream: the cut by bisection and the slot's defined prefix L
//   recover_gaps_kernel       a written frame's gap in front of it: its flag, its pieces for the zero pass
//   recover_totals_kernel     one lane per stream: totals[s][0..7] and what the call adds up
//   recover_records_kernel    the gap records, compacted by the scans over streams and frames
//   recover_decode_kernel     streams_decode_kernel's shape (flac_decode_streams.cpp) with the frame's coded destination;
//                             a dropped or cut frame keeps its lanes idle
//   recover_zero_kernel       one workgroup per piece of a gap: bytes up to the first 16-byte boundary, 16-byte vectors,
//                             bytes behind the last boundary
#include "api_internal.h"
#include "flac_decode_device.h"
#include "stream_batch_core.h"
#include "stream_index.h"
#include "stream_recover_core.h"

namespace flacenc_hip {
namespace {

using namespace streamindex;

using flacdec::FrameRec;
using streamrecover::SegMax;
using Desc = flacenc_hip_stream_desc;
using ull = unsigned long long;

// meta words of this call behind the index's own: gaps, frames dropped, pieces of the zero pass
enum : uint32_t { M_GAPS = M_CLASS, M_DROPPED = M_CLASS + 1, M_PIECES = M_CLASS + 2 };

// what the kernels share: the index's arrays and this call's own over the frame sequence
struct Frames {
  const Desc* descs;
  const uint32_t* perm;
  const uint64_t* origins;  // by stream
  const uint64_t* base;
  const uint32_t *f_node, *f_slot;
  const uint64_t* cand_pos;
  const FrameRec* recs;
  const uint64_t* cand_number;
  const uint32_t* counters;
  uint64_t *P, *emax;        // [F]: coded position; scan value, then its inclusive prefix maximum per stream
  uint64_t *placed, *pl;     // [F] flag, [F + 1] its exclusive scan
  uint32_t* plist;           // [F]: the placed frames in order
  uint64_t *gflag, *pieces;  // [F]: a gap in front of the written frame, the zero pass's workgroups for it
  uint64_t *gp, *pc;         // [F + 1]: their exclusive scans
  uint64_t* acc;             // [n_streams][3]: bytes in chain frames, inner breaks, samples written
  uint32_t* cut;             // [n_streams], by slot: the chain frames in front of the cut
  uint64_t *s_gaps, *gbase;  // [n_streams], [n_streams + 1]: gaps per stream, their exclusive scan
};

__device__ inline uint32_t frame_block(const Frames& f, uint64_t m) { return f.recs[f.f_node[m]].block_size; }

// the end of the written frame in front of written frame m of slot i (the origin if m is the first)
__device__ inline uint64_t prev_written_end(const Frames& f, uint64_t m, uint32_t i, uint64_t origin) {
  if (f.pl[m] == f.pl[f.base[i]]) return origin;
  const uint32_t p = f.plist[f.pl[m] - 1];
  return f.P[p] + frame_block(f, p);
}

__global__ void __launch_bounds__(256) recover_position_kernel(Frames f) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= f.counters[C_FRAMES]) return;
  const uint32_t i = f.f_slot[m], s = f.perm[i], node = f.f_node[m];
  const Desc& d = f.descs[s];
  const uint64_t num = f.cand_number[node];
  const uint64_t P = streamrecover::coded_position(num >> 1, static_cast<uint32_t>(num & 1u), d.max_block_size);
  f.P[m] = P;
  f.emax[m] = streamrecover::scan_value(P, f.recs[node].block_size, f.origins[s]);
  uint64_t prev_end = d.offset;
  if (m != f.base[i]) {
    const uint32_t before = f.f_node[m - 1];
    prev_end = f.cand_pos[before] + f.recs[before].len;
  }
  atomicAdd(reinterpret_cast<ull*>(f.acc + 3 * static_cast<size_t>(s)), static_cast<ull>(f.recs[node].len));
  if (f.cand_pos[node] != prev_end) atomicAdd(reinterpret_cast<ull*>(f.acc + 3 * static_cast<size_t>(s) + 1), 1ull);
}

// ---------------------------------------------------------------- the segmented max-scan
// inclusive scan of x over the workgroup's N threads with streamrecover::combine
template <uint32_t N>
__device__ inline SegMax block_segscan(SegMax x, uint32_t* sh_h, uint64_t* sh_v) {
  const uint32_t t = threadIdx.x;
  sh_h[t] = x.head;
  sh_v[t] = x.v;
  __syncthreads();
  for (uint32_t d = 1; d < N; d <<= 1) {
    SegMax a{0, 0};
    const bool has = t >= d;
    if (has) a = SegMax{sh_h[t - d], sh_v[t - d]};
    __syncthreads();
    if (has) {
      x = streamrecover::combine(a, x);
      sh_h[t] = x.head;
      sh_v[t] = x.v;
    }
    __syncthreads();
  }
  return x;
}

// frame m as an element of the scan; {0, 0}, the identity, behind the sequence
__device__ inline SegMax seg_element(const Frames& f, uint64_t m) {
  if (m >= f.counters[C_FRAMES]) return {0, 0};
  return {m == f.base[f.f_slot[m]] ? 1u : 0u, f.emax[m]};
}

__global__ void __launch_bounds__(256) segmax_reduce_kernel(Frames f, uint32_t* __restrict__ agg_h,
                                                            uint64_t* __restrict__ agg_v) {
  __shared__ uint32_t sh_h[256];
  __shared__ uint64_t sh_v[256];
  const uint64_t m = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const SegMax r = block_segscan<256>(seg_element(f, m), sh_h, sh_v);
  if (threadIdx.x == 255) {
    agg_h[blockIdx.x] = r.head;
    agg_v[blockIdx.x] = r.v;
  }
}

// one workgroup: agg[b] := the combination of every aggregate in front of b (the identity for b == 0)
__global__ void __launch_bounds__(1024) segmax_carry_kernel(uint32_t* __restrict__ agg_h, uint64_t* __restrict__ agg_v,
                                                            uint32_t n) {
  __shared__ uint32_t sh_h[1024];
  __shared__ uint64_t sh_v[1024];
  SegMax carry{0, 0};  // the same in every thread
  for (uint32_t at = 0; at < n; at += 1024u) {
    const uint32_t b = at + threadIdx.x;
    SegMax x{0, 0};
    if (b < n) x = SegMax{agg_h[b], agg_v[b]};
    block_segscan<1024>(x, sh_h, sh_v);
    SegMax before = carry;
    if (threadIdx.x) before = streamrecover::combine(carry, SegMax{sh_h[threadIdx.x - 1], sh_v[threadIdx.x - 1]});
    if (b < n) {
      agg_h[b] = before.head;
      agg_v[b] = before.v;
    }
    carry = streamrecover::combine(carry, SegMax{sh_h[1023], sh_v[1023]});
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) segmax_apply_kernel(Frames f, const uint32_t* __restrict__ agg_h,
                                                           const uint64_t* __restrict__ agg_v) {
  __shared__ uint32_t sh_h[256];
  __shared__ uint64_t sh_v[256];
  const uint64_t m = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const SegMax r = block_segscan<256>(seg_element(f, m), sh_h, sh_v);
  if (m < f.counters[C_FRAMES])
    f.emax[m] = streamrecover::combine(SegMax{agg_h[blockIdx.x], agg_v[blockIdx.x]}, r).v;
}

// ---------------------------------------------------------------- placement, cut, gaps
__global__ void __launch_bounds__(256) recover_place_kernel(Frames f) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= f.counters[C_FRAMES]) return;
  const uint32_t i = f.f_slot[m], s = f.perm[i];
  const uint64_t origin = f.origins[s];
  const uint64_t prev_max = m == f.base[i] ? origin : f.emax[m - 1];
  f.placed[m] = streamrecover::is_placed(f.P[m], frame_block(f, m), f.descs[s].max_block_size, origin, prev_max) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) recover_list_kernel(Frames f) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < f.counters[C_FRAMES] && f.placed[m]) f.plist[f.pl[m]] = m;
}

// L of slot i cut at `cut` chain frames: the end of its last written frame from the origin on
__device__ inline uint64_t defined_samples(const Frames& f, uint32_t i, uint64_t cut, uint64_t origin) {
  const uint64_t first = f.base[i];
  if (f.pl[first + cut] == f.pl[first]) return 0;
  const uint32_t last = f.plist[f.pl[first + cut] - 1];
  return f.P[last] + frame_block(f, last) - origin;
}

// one lane per slot: the cut and the bytes of the slot's defined prefix (s_bytes, by stream)
__global__ void __launch_bounds__(256) recover_cut_kernel(Frames f, uint32_t n_streams, uint64_t* __restrict__ s_bytes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const uint32_t s = f.perm[i];
  uint64_t cut = 0, bytes = 0;
  if (!f.counters[C_ERR]) {
    const Desc& d = f.descs[s];
    const uint32_t W = d.channels * d.bytes_per_sample;
    const uint64_t first = f.base[i], origin = f.origins[s];
    cut = streamrecover::cut_frames(f.emax, first, f.base[i + 1] - first, origin, W, d.out_capacity);
    bytes = defined_samples(f, i, cut, origin) * W;
  }
  f.cut[i] = static_cast<uint32_t>(cut);
  s_bytes[s] = bytes;
}

__global__ void __launch_bounds__(256) recover_gaps_kernel(Frames f) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= f.counters[C_FRAMES]) return;
  const uint32_t i = f.f_slot[m], s = f.perm[i];
  uint64_t gap = 0, pieces = 0;
  if (f.placed[m] && m - f.base[i] < f.cut[i]) {
    const Desc& d = f.descs[s];
    gap = streamrecover::gap_before(f.P[m], prev_written_end(f, m, i, f.origins[s]));
    pieces = streamrecover::pieces_of(gap * d.channels * d.bytes_per_sample);
    atomicAdd(reinterpret_cast<ull*>(f.acc + 3 * static_cast<size_t>(s) + 2), static_cast<ull>(frame_block(f, m)));
    if (gap) atomicAdd(reinterpret_cast<ull*>(f.s_gaps + s), 1ull);
  }
  f.gflag[m] = gap ? 1u : 0u;
  f.pieces[m] = pieces;
}

// one lane per slot: the stream's totals and what the call adds up
__global__ void __launch_bounds__(256) recover_totals_kernel(Frames f, uint32_t n_streams,
                                                             const uint64_t* __restrict__ s_end,
                                                             uint64_t* __restrict__ totals, uint64_t* __restrict__ meta) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const uint32_t s = f.perm[i];
  uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!f.counters[C_ERR]) {
    const Desc& d = f.descs[s];
    const uint64_t first = f.base[i], count = f.base[i + 1] - first, cut = f.cut[i];
    const uint64_t* acc = f.acc + 3 * static_cast<size_t>(s);
    t[0] = f.pl[first + cut] - f.pl[first];
    t[1] = defined_samples(f, i, cut, f.origins[s]);
    t[2] = t[1] - acc[2];
    t[3] = count - (f.pl[first + count] - f.pl[first]);
    t[4] = d.n_bytes - acc[0];
    t[5] = acc[1] + (count ? (s_end[s] != d.offset + d.n_bytes ? 1u : 0u) : (d.n_bytes ? 1u : 0u));
    t[6] = f.pl[first + count] != f.pl[first + cut] ? FLACENC_HIP_DECODE_NO_ROOM : 0;
    if (t[0]) atomicAdd(reinterpret_cast<ull*>(meta + M_FRAMES), static_cast<ull>(t[0]));
    if (t[1]) atomicAdd(reinterpret_cast<ull*>(meta + M_SAMPLES), static_cast<ull>(t[1]));
    if (f.s_gaps[s]) atomicAdd(reinterpret_cast<ull*>(meta + M_GAPS), static_cast<ull>(f.s_gaps[s]));
    if (t[3]) atomicAdd(reinterpret_cast<ull*>(meta + M_DROPPED), static_cast<ull>(t[3]));
    if (i == 0) meta[M_PIECES] = f.pc[f.counters[C_FRAMES]];
  }
  for (uint32_t k = 0; k < 8; ++k) totals[8 * static_cast<size_t>(s) + k] = t[k];
}

__global__ void __launch_bounds__(256) recover_records_kernel(Frames f, uint64_t* __restrict__ gaps, uint64_t max_gaps) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= f.counters[C_FRAMES] || !f.gflag[m]) return;
  const uint32_t i = f.f_slot[m], s = f.perm[i];
  const uint64_t at = f.gbase[s] + (f.gp[m] - f.gp[f.base[i]]);
  if (at >= max_gaps) return;
  const uint64_t origin = f.origins[s], prev_end = prev_written_end(f, m, i, origin);
  gaps[3 * at + 0] = s;
  gaps[3 * at + 1] = prev_end - origin;
  gaps[3 * at + 2] = f.P[m] - prev_end;
}

// ---------------------------------------------------------------- decode and zero pass
// streams_decode_kernel with the frame's coded destination: the frames [m_lo, m_hi) all have `channels` channels; a
// frame that is dropped or lies behind its stream's cut keeps its lanes idle (bs == 0), as both lanes of a pair do
template <bool DEEP>
__global__ void __launch_bounds__(256) recover_decode_kernel(const uint8_t* __restrict__ bytes, Frames f, uint32_t m_lo,
                                                             uint32_t m_hi, uint32_t channels,
                                                             const uint64_t* __restrict__ where,
                                                             uint8_t* __restrict__ out) {
  const uint32_t per_block = blockDim.x / channels;  // frames never straddle workgroups
  const uint32_t lf = threadIdx.x / channels, c = threadIdx.x % channels;
  const uint64_t m = static_cast<uint64_t>(m_lo) + static_cast<uint64_t>(blockIdx.x) * per_block + lf;
  uint32_t bs = 0, ch_tag = 0, flen = 0, start = 0, bps = 0, B = 1;
  const uint8_t* fp = bytes;
  uint8_t* dst = out;
  if (lf < per_block && m < m_hi) {
    const uint32_t i = f.f_slot[m], s = f.perm[i];
    if (f.placed[m] && m - f.base[i] < f.cut[i]) {
      const Desc& d = f.descs[s];
      const uint32_t node = f.f_node[m];
      const FrameRec& r = f.recs[node];
      bs = r.block_size;
      ch_tag = (r.info >> 4) & 15u;
      flen = r.len;
      start = r.sub_bit[c];
      bps = d.bits_per_sample;
      B = d.bytes_per_sample;
      fp = bytes + f.cand_pos[node];
      dst = out + (where ? where[s] : d.out_offset) + (f.P[m] - f.origins[s]) * (static_cast<uint64_t>(channels) * B);
    }
  }
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const int bucket = lane_bucket(fp, flen, start, bs, sbps);
  AT_WAVE_DECODER(DEEP, bucket, flacdec::needs_wide(bps),
                  write_pcm<MAXP, WIDE>(fp, flen, start, bs, 0, bs, sbps, ch_tag, c, channels, B, dst, ON));
}

// Workgroup `blockIdx.x` clears piece q of the gap in front of frame m, pc[m] <= blockIdx.x < pc[m + 1]: bytes
// [q * PIECE, (q + 1) * PIECE) of the gap, cut at its end -- a range of any alignment that holds no byte of a frame.
__global__ void __launch_bounds__(256) recover_zero_kernel(Frames f, const uint64_t* __restrict__ where,
                                                           uint8_t* __restrict__ out) {
  const uint32_t n = f.counters[C_FRAMES];
  const uint64_t blk = blockIdx.x;
  if (blk >= f.pc[n]) return;
  uint32_t lo = 0, hi = n;  // the first frame whose pieces start behind blk
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (f.pc[mid] <= blk) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t m = lo - 1;
  const uint32_t i = f.f_slot[m], s = f.perm[i];
  const Desc& d = f.descs[s];
  const uint64_t W = static_cast<uint64_t>(d.channels) * d.bytes_per_sample, origin = f.origins[s];
  const uint64_t g_lo = (prev_written_end(f, m, i, origin) - origin) * W, g_hi = (f.P[m] - origin) * W;
  uint64_t b_lo = g_lo + (blk - f.pc[m]) * streamrecover::PIECE, b_hi = b_lo + streamrecover::PIECE;
  if (b_hi > g_hi) b_hi = g_hi;
  uint8_t* slot = out + (where ? where[s] : d.out_offset);
  const uint64_t a_lo = reinterpret_cast<uintptr_t>(slot + b_lo), a_hi = reinterpret_cast<uintptr_t>(slot + b_hi);
  const streamrecover::ZeroSplit z = streamrecover::zero_split(a_lo, a_hi);
  const uint32_t t = threadIdx.x;  // at most 15 head bytes, PIECE / 16 vectors and 15 tail bytes: one of each per lane
  if (t < z.head) reinterpret_cast<uint8_t*>(a_lo)[t] = 0;
  if (t < z.vectors) reinterpret_cast<uint4*>(a_lo + z.head)[t] = make_uint4(0, 0, 0, 0);
  if (t < z.tail) reinterpret_cast<uint8_t*>(a_hi - z.tail)[t] = 0;
}

}  // namespace

// The three launches of the segmented max-scan over a frame sequence of at most max_frames elements (api_internal.h):
// recover_streams_impl below and flacenc_hip_debug_segmax_scan (api_debug_hooks.cpp) both come through here.
hipError_t launch_segmax_scan(uint64_t* plan, const uint32_t* f_slot, const uint64_t* base, uint64_t* emax,
                              const uint32_t* counters, size_t max_frames, uint32_t* agg_h, uint64_t* agg_v,
                              hipStream_t stream) {
  Frames f{};  // the kernels read these four fields and no other
  f.f_slot = f_slot;
  f.base = base;
  f.emax = emax;
  f.counters = counters;
  const size_t NB = ceil_div(max_frames, 256);
  const dim3 per_frame(max_frames ? NB : 1), wg(256);
  COUNTED_LAUNCH(plan, segmax_reduce_kernel, per_frame, wg, 0, stream, f, agg_h, agg_v);
  COUNTED_LAUNCH(plan, segmax_carry_kernel, dim3(1), dim3(1024), 0, stream, agg_h, agg_v,
                 static_cast<uint32_t>(max_frames ? NB : 0));
  COUNTED_LAUNCH(plan, segmax_apply_kernel, per_frame, wg, 0, stream, f, agg_h, agg_v);
  return hipGetLastError();
}

namespace {

int recover_streams_impl(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                         size_t n_streams, const uint64_t* origins, size_t max_frames, uint8_t* out, uint64_t out_bytes,
                         uint64_t* totals, uint64_t* gaps, size_t max_gaps, uint64_t call_totals[4], int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  uint64_t* plan = h->last_recover_plan;  // launches, synchronisations, transfers, channel classes
  plan[0] = plan[1] = plan[2] = plan[3] = 0;
  if (!call_limits_ok(memory_kind, n_streams, max_frames, n_bytes) || !bytes || !streams || !out || !totals ||
      !call_totals || (!gaps && max_gaps)) {
    h->last_error = "recover_streams: null pointer (gaps with max_gaps > 0 included), unknown memory kind, more than 2^24 "
                    "streams, max_frames above 2^30 or n_bytes >= 16 TiB";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const Desc* table = static_cast<const Desc*>(streams);
  int rc = streambatch::check_streams(table, n_streams, n_bytes, out_bytes, h->max_bps);
  if (rc == FLACENC_HIP_ERR_UNSUPPORTED) {
    h->last_error = "recover_streams: a stream's bits_per_sample not in 4..=24 (4..=32 with "
                    "flacenc_hip_set_max_bits_per_sample)";
    return rc;
  }
  if (rc != FLACENC_HIP_OK) {
    h->last_error = "recover_streams: spans not ascending, overlapping or past n_bytes, a slot past out_bytes, channels "
                    "not in 1..=8, max_block_size not in 1..=65536 or bytes_per_sample not in ceil(bits / 8)..=4";
    return rc;
  }
  call_totals[0] = call_totals[1] = call_totals[2] = call_totals[3] = 0;
  if (n_streams == 0) return FLACENC_HIP_OK;
  const bool host = memory_kind == FLACENC_HIP_MEM_HOST;
  const uint32_t ns = static_cast<uint32_t>(n_streams);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;

  // ---- this call's scratch behind the index's ----
  const size_t F = max_frames, NB = ceil_div(F, 256);
  const size_t gap_room = max_gaps < F ? max_gaps : F;  // a gap lies in front of a written frame
  size_t need = 0;
  auto take = [&need](size_t bytes_) {
    const size_t at = need;
    need += a256(bytes_ + 8);
    return at;
  };
  const size_t o_P = take(F * 8), o_emax = take(F * 8), o_placed = take(F * 8), o_pl = take((F + 1) * 8);
  const size_t o_plist = take(F * 4), o_gflag = take(F * 8), o_pieces = take(F * 8), o_gp = take((F + 1) * 8);
  const size_t o_pc = take((F + 1) * 8), o_aggh = take(NB * 4), o_aggv = take(NB * 8);
  const size_t o_cut = take(n_streams * 4), o_gbase = take((n_streams + 1) * 8);
  const size_t o_acc = take(n_streams * 32);  // acc[n][3] | s_gaps[n]: cleared together
  const size_t o_gaps = host ? take(gap_room * 24) : 0;

  // ---- the resynchronising index; the origins go up with the table; behind `base`, host memory: totals | where ----
  std::vector<uint64_t> zeros;
  if (!origins) {
    zeros.assign(n_streams, 0);
    origins = zeros.data();
  }
  Request rq{};
  rq.bytes = bytes;
  rq.n_bytes = n_bytes;
  rq.table = table;
  rq.n_streams = n_streams;
  rq.max_frames = max_frames;
  rq.host = host;
  rq.who = "recover_streams";
  rq.extra_words = host ? 8 * n_streams + (n_streams + 1) : 0;
  rq.pinned_tail = host ? gap_room * 24 : 0;
  rq.extra_table = origins;
  rq.extra_table_bytes = n_streams * 8;
  rq.extra_scratch = need;
  rq.resync = true;
  Index ix;
  Drain drain{h};
  if ((rc = build(h, plan, rq, ix)) != FLACENC_HIP_OK) return rc;
  const size_t result_words = ix.result_words;
  uint64_t* d_totals = host ? ix.extra : totals;
  uint64_t* where = host ? ix.extra + 8 * n_streams : nullptr;
  uint64_t* d_gaps = host ? reinterpret_cast<uint64_t*>(ix.scratch + o_gaps) : gaps;
  char* X = ix.scratch;
  Frames f;
  f.descs = ix.descs;
  f.perm = ix.perm;
  f.origins = reinterpret_cast<const uint64_t*>(ix.extra_table);
  f.base = ix.base;
  f.f_node = ix.f_node;
  f.f_slot = ix.f_slot;
  f.cand_pos = ix.cand_pos;
  f.recs = ix.recs;
  f.cand_number = ix.cand_number;
  f.counters = ix.counters;
  f.P = reinterpret_cast<uint64_t*>(X + o_P);
  f.emax = reinterpret_cast<uint64_t*>(X + o_emax);
  f.placed = reinterpret_cast<uint64_t*>(X + o_placed);
  f.pl = reinterpret_cast<uint64_t*>(X + o_pl);
  f.plist = reinterpret_cast<uint32_t*>(X + o_plist);
  f.gflag = reinterpret_cast<uint64_t*>(X + o_gflag);
  f.pieces = reinterpret_cast<uint64_t*>(X + o_pieces);
  f.gp = reinterpret_cast<uint64_t*>(X + o_gp);
  f.pc = reinterpret_cast<uint64_t*>(X + o_pc);
  f.acc = reinterpret_cast<uint64_t*>(X + o_acc);
  f.s_gaps = f.acc + 3 * n_streams;
  f.cut = reinterpret_cast<uint32_t*>(X + o_cut);
  f.gbase = reinterpret_cast<uint64_t*>(X + o_gbase);
  uint32_t* agg_h = reinterpret_cast<uint32_t*>(X + o_aggh);
  uint64_t* agg_v = reinterpret_cast<uint64_t*>(X + o_aggv);
  const uint32_t* n_frames = ix.counters + C_FRAMES;
  const dim3 per_frame(F ? NB : 1), per_stream(ceil_div(ns, 256)), wg(256);

  HIP_TRY(h, hipMemsetAsync(f.acc, 0, n_streams * 32, st));
  // ---- positions, the prefix maximum per stream, placement ----
  COUNTED_LAUNCH(plan, recover_position_kernel, per_frame, wg, 0, st, f);
  HIP_TRY(h, launch_segmax_scan(plan, f.f_slot, f.base, f.emax, f.counters, F, agg_h, agg_v, st));
  COUNTED_LAUNCH(plan, recover_place_kernel, per_frame, wg, 0, st, f);
  HIP_TRY(h, launch_scan2_dev(f.placed, nullptr, F, n_frames, f.pl, nullptr, st));
  ++plan[0];
  COUNTED_LAUNCH(plan, recover_list_kernel, per_frame, wg, 0, st, f);
  // ---- the cut, the gaps, the totals and the records ----
  COUNTED_LAUNCH(plan, recover_cut_kernel, per_stream, wg, 0, st, f, ns, ix.s_bytes);
  COUNTED_LAUNCH(plan, recover_gaps_kernel, per_frame, wg, 0, st, f);
  HIP_TRY(h, launch_scan2_dev(f.gflag, f.pieces, F, n_frames, f.gp, f.pc, st));
  ++plan[0];
  HIP_TRY(h, launch_scan2(f.s_gaps, nullptr, ns, f.gbase, nullptr, st));
  ++plan[0];
  COUNTED_LAUNCH(plan, recover_totals_kernel, per_stream, wg, 0, st, f, ns, ix.s_end, d_totals, ix.meta);
  if (host) {
    HIP_TRY(h, launch_scan2(ix.s_bytes, nullptr, ns, where, nullptr, st));
    ++plan[0];
  }
  HIP_TRY(h, hipGetLastError());
  const uint64_t* r_meta = static_cast<const uint64_t*>(h->pin_meta[0]);
  HIP_TRY(h, hipMemcpyAsync(h->pin_meta[0], ix.meta, result_words * 8, hipMemcpyDeviceToHost, st));
  ++plan[2];
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  const uint64_t* r_base = r_meta + M_WORDS;
  const uint64_t* r_totals = r_base + (n_streams + 1);
  const uint64_t* r_where = r_totals + 8 * n_streams;
  if (r_meta[M_ERR]) {  // nothing reaches `out` or `gaps`; every stream's totals are zero (the kernel wrote them so)
    if (host) std::memcpy(totals, r_totals, n_streams * 64);
    call_totals[0] = FLACENC_HIP_INDEX_ERROR;
    drain.armed = false;
    return FLACENC_HIP_OK;
  }
  const uint64_t n_pieces = r_meta[M_PIECES];
  if (n_pieces > 0x7FFFFFFFull) {
    h->last_error = "recover_streams: more than 8 TiB of silence in one call";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }

  // ---- decode at the coded positions: one launch per channel count present; then the holes ----
  uint8_t* d_out = out;
  const uint64_t pcm_bytes = host ? r_where[n_streams] : 0;
  if (host) {
    if ((rc = ensure(h, h->d_cont[0], static_cast<size_t>(pcm_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_out = static_cast<uint8_t*>(h->d_cont[0].ptr);
  }
  const bool deep = any_deep_stream(table, n_streams);
  // (the records: behind the one place the call can still end without having written anything)
  COUNTED_LAUNCH(plan, recover_records_kernel, per_frame, wg, 0, st, f, d_gaps, static_cast<uint64_t>(host ? gap_room : max_gaps));
  for (uint32_t c = 1; c <= 8; ++c) {
    if (ix.slot_lo[c] == ix.slot_lo[c + 1]) continue;
    const uint32_t m_lo = static_cast<uint32_t>(r_base[ix.slot_lo[c]]), m_hi = static_cast<uint32_t>(r_base[ix.slot_lo[c + 1]]);
    const uint32_t per_block = 256 / c;
    const dim3 grid(m_hi > m_lo ? ceil_div(m_hi - m_lo, per_block) : 1), block(per_block * c);
    if (deep)
      COUNTED_LAUNCH(plan, recover_decode_kernel<true>, grid, block, 0, st, ix.d_bytes, f, m_lo, m_hi, c, where, d_out);
    else
      COUNTED_LAUNCH(plan, recover_decode_kernel<false>, grid, block, 0, st, ix.d_bytes, f, m_lo, m_hi, c, where, d_out);
  }
  // (a call without gaps still counts the launch: the plan does not depend on the damage)
  COUNTED_LAUNCH(plan, recover_zero_kernel, dim3(n_pieces ? static_cast<uint32_t>(n_pieces) : 1), wg, 0, st, f, where,
                 d_out);
  HIP_TRY(h, hipGetLastError());
  const uint64_t n_gaps = r_meta[M_GAPS], gaps_down = n_gaps < gap_room ? n_gaps : gap_room;
  char* p_gaps = static_cast<char*>(h->pin_meta[0]) + result_words * 8;
  if (host) {
    // always counted, so that the plan does not depend on the damage
    if (gaps_down) HIP_TRY(h, hipMemcpyAsync(p_gaps, d_gaps, gaps_down * 24, hipMemcpyDeviceToHost, st));
    ++plan[2];
    if ((rc = download_pcm(h, plan, "recover_streams", d_out, pcm_bytes)) != FLACENC_HIP_OK) return rc;
  }
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  drain.armed = false;
  if (host) {
    const uint8_t* staged = static_cast<const uint8_t*>(h->pin_out[0]);
    for (size_t s = 0; s < n_streams; ++s) {
      const uint64_t n = r_where[s + 1] - r_where[s];
      if (n) h->copy_pool->copy(out + table[s].out_offset, staged + r_where[s], static_cast<size_t>(n));
    }
    std::memcpy(totals, r_totals, n_streams * 64);
    if (gaps_down) std::memcpy(gaps, p_gaps, gaps_down * 24);
  }
  call_totals[0] = r_meta[M_FRAMES];
  call_totals[1] = r_meta[M_SAMPLES];
  call_totals[2] = n_gaps;
  call_totals[3] = r_meta[M_DROPPED];
  return FLACENC_HIP_OK;
}

}  // namespace
}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" int flacenc_hip_recover_streams(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                           const void* streams, size_t n_streams, const uint64_t* origins,
                                           size_t max_frames, uint8_t* out, uint64_t out_bytes, uint64_t* totals,
                                           uint64_t* gaps, size_t max_gaps, uint64_t call_totals[4], int memory_kind) {
  return recover_streams_impl(h, bytes, n_bytes, streams, n_streams, origins, max_frames, out, out_bytes, totals, gaps,
                              max_gaps, call_totals, memory_kind);
}
