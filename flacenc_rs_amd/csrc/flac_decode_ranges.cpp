// flac_decode_ranges.cpp -- flacenc_hip_decode_ranges: sample ranges of a batch of FLAC streams to packed PCM in one
// call, with a number of launches, synchronisations and transfers that does not depend on the number of streams or of
// ranges.
//
// The segmented index is flacenc_hip_decode_streams' own (stream_index.h, stream_index.cpp): every stream's verified
// chain, every chain frame enumerated, and the scans of PCM bytes and of frames with a status over the frame sequence.
// Positions are read off the scan of PCM bytes (stream_ranges_core.h).  On top of it:
//   ranges_streams_kernel    one lane per stream: the chain frames that decode, S (its samples), W (why it stops) and
//                            where the chain stopped
//   ranges_locate_kernel     one lane per range: bisects its stream's positions for the frame that holds first_sample
//                            and the frame that holds the last wanted sample below S; writes the range's frame count,
//                            its totals and its seek point
//   one scan                 range-frame bases and (host memory) where each range's PCM starts in compact staging
//   ranges_verdict_kernel    one thread: more range-frames than max_frames end the call with the flag
//   ranges_enumerate_kernel  one lane per range-frame: its range, by bisection, and its chain frame
//   ranges_decode_kernel     one launch per channel count present among the ranges' streams (ranges are numbered in
//                            `rslot` order: the range table sorted by their stream's channel count), with the lane rules
//                            of streams_decode_kernel and its writer (write_pcm, flac_decode_device.h) with a window per
//                            frame: the recurrence runs from the frame's first sample -- it is serial -- to the last
//                            sample wanted, and only samples inside the range are stored
// flacenc_hip_decode_ranges_planar is the same call with another slot: rows of 4-byte elements,
// channel after channel (stream_planar_core.h).  It differs in
//   ranges_decode_planar_kernel  in place of ranges_decode_kernel: the same lanes with the planar writer (write_planar,
//                            flac_decode_device.h): elements converted in registers, staged in LDS and stored as
//                            16-byte vectors wherever the row's address allows
//   ranges_zero_kernel       device memory only, one launch for all ranges: elements [written, n_samples) of every row
//                            (in host memory the rows come back packed and the host zeroes behind them)
#include "api_internal.h"
#include "flac_decode_device.h"
#include "stream_batch_core.h"
#include "stream_index.h"
#include "stream_ranges_core.h"

namespace flacenc_hip {
namespace {

using namespace streamindex;
using flacdec::FrameRec;
using Desc = flacenc_hip_stream_desc;
using Range = flacenc_hip_range_desc;

// per stream, what the ranges on it share
struct StreamEnd {
  uint64_t first;     // its first frame in the sequence
  uint64_t good;      // the chain frames in front of the first one with a status
  uint64_t why;       // W: 0, CHAIN, or the status of frame `good`
  uint64_t consumed;  // where the chain stopped, from the span's start
};

// range-frames in front of the ranges of c channels, c = 1 .. 9, in rslot order
struct ClassLo {
  uint32_t lo[10];
};

__global__ void __launch_bounds__(256) ranges_streams_kernel(const Desc* __restrict__ descs,
                                                             const uint32_t* __restrict__ perm, uint32_t n_streams,
                                                             const uint64_t* __restrict__ base,
                                                             const uint64_t* __restrict__ pcm,
                                                             const uint64_t* __restrict__ bad,
                                                             const uint32_t* __restrict__ f_node,
                                                             const uint64_t* __restrict__ cand_pos,
                                                             const uint64_t* __restrict__ s_end,
                                                             const uint32_t* __restrict__ s_why,
                                                             const uint32_t* __restrict__ counters,
                                                             StreamEnd* __restrict__ ends) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const uint32_t s = perm[i];
  StreamEnd e{0, 0, 0, 0};
  if (!counters[C_ERR]) {
    const Desc& d = descs[s];
    const uint64_t first = base[i], count = base[i + 1] - first;
    e.first = first;
    e.good = streambatch::accepted_frames(pcm, bad, first, count, ~0ull);
    if (e.good < count) {  // a frame of the chain with a status: a block above the stream's max_block_size
      e.why = FLACENC_HIP_DECODE_UNSUPPORTED;
      e.consumed = cand_pos[f_node[first + e.good]] - d.offset;
    } else {
      e.why = s_why[s];
      e.consumed = s_end[s] - d.offset;
    }
  }
  ends[s] = e;
}

// lane q: the range rperm[q].  r_bytes is what the range's samples take in the compact staging of the host path: packed
// PCM, or (PLANAR) `channels` rows of 4-byte elements
template <bool PLANAR>
__global__ void __launch_bounds__(256) ranges_locate_kernel(const Desc* __restrict__ descs,
                                                            const Range* __restrict__ ranges,
                                                            const uint32_t* __restrict__ rperm, uint32_t n_ranges,
                                                            const StreamEnd* __restrict__ ends,
                                                            const uint64_t* __restrict__ pcm,
                                                            const uint32_t* __restrict__ f_node,
                                                            const uint64_t* __restrict__ cand_pos,
                                                            const uint32_t* __restrict__ counters,
                                                            uint64_t* __restrict__ r_frames,
                                                            uint64_t* __restrict__ r_bytes,
                                                            uint64_t* __restrict__ r_first,
                                                            uint64_t* __restrict__ r_written,
                                                            uint64_t* __restrict__ totals, uint64_t* __restrict__ meta) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_ranges) return;
  const uint32_t r = rperm[q];
  const Range x = ranges[r];
  const Desc& d = descs[x.stream];
  const uint64_t fb = static_cast<uint64_t>(d.channels) * d.bytes_per_sample;
  uint64_t frames = 0, written = 0, first_frame = 0, why = 0, seek_off = 0, seek_pos = 0;
  if (!counters[C_ERR]) {
    const StreamEnd e = ends[x.stream];
    const streamranges::Located l = streamranges::locate(pcm, e.first, e.good, fb, x.first_sample, x.n_samples);
    frames = l.frames;
    written = l.written;
    first_frame = e.first + l.f0;
    why = streamranges::stop_reason(written, x.n_samples, e.why);
    seek_pos = streamranges::position(pcm, e.first, l.f0, fb);
    seek_off = l.f0 < e.good ? cand_pos[f_node[first_frame]] - d.offset : e.consumed;
    if (written) atomicAdd(reinterpret_cast<unsigned long long*>(meta + M_SAMPLES), static_cast<unsigned long long>(written));
  }
  r_frames[q] = frames;
  r_bytes[q] = PLANAR ? streamplanar::slot_bytes(d.channels, written) : written * fb;
  r_first[q] = first_frame;
  r_written[q] = written;
  totals[4 * static_cast<size_t>(r) + 0] = written;
  totals[4 * static_cast<size_t>(r) + 1] = why;
  totals[4 * static_cast<size_t>(r) + 2] = seek_off;
  totals[4 * static_cast<size_t>(r) + 3] = seek_pos;
}

// one thread: more range-frames than max_frames end the call with the flag; else the range-frames in front of every
// channel class go where the host reads them
__global__ void ranges_verdict_kernel(const uint64_t* __restrict__ r_base, uint32_t n_ranges, uint64_t max_frames,
                                      ClassLo rslot_lo, uint32_t* __restrict__ counters, uint64_t* __restrict__ meta) {
  const uint64_t total = r_base[n_ranges];
  if (counters[C_ERR]) {
    counters[C_FRAMES] = 0;
    return;
  }
  const uint32_t err = total > max_frames;
  counters[C_ERR] = err;
  counters[C_FRAMES] = err ? 0u : static_cast<uint32_t>(total);  // from here on: the range-frames
  meta[M_ERR] = err;
  meta[M_FRAMES] = total;
  for (uint32_t c = 0; c < 10; ++c) meta[M_CLASS + c] = r_base[rslot_lo.lo[c]];
}

__global__ void __launch_bounds__(256) ranges_enumerate_kernel(const uint64_t* __restrict__ r_base, uint32_t n_ranges,
                                                               const uint64_t* __restrict__ r_first,
                                                               const uint32_t* __restrict__ counters,
                                                               uint32_t* __restrict__ rf_range,
                                                               uint32_t* __restrict__ rf_frame) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= counters[C_FRAMES]) return;
  const uint32_t q = streambatch::slot_of_frame(r_base, n_ranges, k);
  rf_range[k] = q;
  rf_frame[k] = static_cast<uint32_t>(r_first[q] + (k - r_base[q]));
}

// ---------------------------------------------------------------- reconstruction: one lane per subframe
// The range-frames [k_lo, k_hi) all belong to streams of `channels` channels; lane (range-frame, c) as in
// streams_decode_kernel.  A range's PCM starts at out + where[q] (`where` given: the compact staging of the host path)
// or at out + its out_offset.  DEEP: see AT_WAVE_DECODER.
template <bool DEEP>
__global__ void __launch_bounds__(256) ranges_decode_kernel(const uint8_t* __restrict__ bytes,
                                                            const Desc* __restrict__ descs,
                                                            const Range* __restrict__ ranges,
                                                            const uint32_t* __restrict__ rperm,
                                                            const uint64_t* __restrict__ base,
                                                            const uint64_t* __restrict__ pcm,
                                                            const uint32_t* __restrict__ f_node,
                                                            const uint32_t* __restrict__ f_slot,
                                                            const uint32_t* __restrict__ rf_range,
                                                            const uint32_t* __restrict__ rf_frame,
                                                            const uint64_t* __restrict__ r_written,
                                                            const uint64_t* __restrict__ cand_pos,
                                                            const FrameRec* __restrict__ recs, uint32_t k_lo,
                                                            uint32_t k_hi, uint32_t channels,
                                                            const uint64_t* __restrict__ where, uint8_t* __restrict__ out) {
  const uint32_t per_block = blockDim.x / channels;  // frames never straddle workgroups
  const uint32_t lf = threadIdx.x / channels, c = threadIdx.x % channels;
  const uint64_t k = static_cast<uint64_t>(k_lo) + static_cast<uint64_t>(blockIdx.x) * per_block + lf;
  uint32_t bs = 0, skip = 0, take = 0, ch_tag = 0, flen = 0, start = 0, bps = 0, B = 1;
  const uint8_t* fp = bytes;
  uint8_t* dst = out;
  if (lf < per_block && k < k_hi) {
    const uint32_t q = rf_range[k], m = rf_frame[k];
    const Range& x = ranges[rperm[q]];
    const Desc& d = descs[x.stream];
    const uint32_t node = f_node[m];
    const FrameRec& r = recs[node];
    const uint64_t fb = static_cast<uint64_t>(d.channels) * d.bytes_per_sample;
    const uint64_t pos = (pcm[m] - pcm[base[f_slot[m]]]) / fb;
    const streamranges::Window w = streamranges::window(pos, r.block_size, x.first_sample, x.first_sample + r_written[q]);
    bs = r.block_size;
    skip = w.skip;
    take = w.take;
    ch_tag = (r.info >> 4) & 15u;
    flen = r.len;
    start = r.sub_bit[c];
    bps = d.bits_per_sample;
    B = d.bytes_per_sample;
    fp = bytes + cand_pos[node];
    dst = out + (where ? where[q] : x.out_offset) + w.dst * fb;
  }
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const int bucket = lane_bucket(fp, flen, start, bs, sbps);
  AT_WAVE_DECODER(DEEP, bucket, flacdec::needs_wide(bps),
                  write_pcm<MAXP, WIDE>(fp, flen, start, bs, skip, take, sbps, ch_tag, c, channels, B, dst, ON));
}

// The planar form: the same lanes under the same rules, each with its row of the range's slot -- channel c's n_samples
// elements (`where` given: its `written` elements, the rows packed back to back in compact staging) -- and the planar
// writer (write_planar, flac_decode_device.h) in place of write_pcm.
template <bool DEEP>
__global__ void __launch_bounds__(256) ranges_decode_planar_kernel(const uint8_t* __restrict__ bytes,
                                                                   const Desc* __restrict__ descs,
                                                                   const Range* __restrict__ ranges,
                                                                   const uint32_t* __restrict__ rperm,
                                                                   const uint64_t* __restrict__ base,
                                                                   const uint64_t* __restrict__ pcm,
                                                                   const uint32_t* __restrict__ f_node,
                                                                   const uint32_t* __restrict__ f_slot,
                                                                   const uint32_t* __restrict__ rf_range,
                                                                   const uint32_t* __restrict__ rf_frame,
                                                                   const uint64_t* __restrict__ r_written,
                                                                   const uint64_t* __restrict__ cand_pos,
                                                                   const FrameRec* __restrict__ recs, uint32_t k_lo,
                                                                   uint32_t k_hi, uint32_t channels,
                                                                   const uint64_t* __restrict__ where,
                                                                   uint32_t sample_format, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t stage_all[256 * kPlanarStage];
  const uint32_t per_block = blockDim.x / channels;  // frames never straddle workgroups
  const uint32_t lf = threadIdx.x / channels, c = threadIdx.x % channels;
  const uint64_t k = static_cast<uint64_t>(k_lo) + static_cast<uint64_t>(blockIdx.x) * per_block + lf;
  uint32_t bs = 0, skip = 0, take = 0, ch_tag = 0, flen = 0, start = 0, bps = 1;
  const uint8_t* fp = bytes;
  uint8_t* dst = out;
  if (lf < per_block && k < k_hi) {
    const uint32_t q = rf_range[k], m = rf_frame[k];
    const Range& x = ranges[rperm[q]];
    const Desc& d = descs[x.stream];
    const uint32_t node = f_node[m];
    const FrameRec& r = recs[node];
    const uint64_t fb = static_cast<uint64_t>(d.channels) * d.bytes_per_sample;
    const uint64_t pos = (pcm[m] - pcm[base[f_slot[m]]]) / fb;
    const uint64_t written = r_written[q];
    const streamranges::Window w = streamranges::window(pos, r.block_size, x.first_sample, x.first_sample + written);
    bs = r.block_size;
    skip = w.skip;
    take = w.take;
    ch_tag = (r.info >> 4) & 15u;
    flen = r.len;
    start = r.sub_bit[c];
    bps = d.bits_per_sample;
    fp = bytes + cand_pos[node];
    dst = out + (where ? streamplanar::element_offset(where[q], written, c, w.dst)
                       : streamplanar::element_offset(x.out_offset, x.n_samples, c, w.dst));
  }
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const float scale = streamplanar::scale_of(bps);
  uint32_t* stage = stage_all + threadIdx.x * kPlanarStage;
  const int bucket = lane_bucket(fp, flen, start, bs, sbps);
  AT_WAVE_DECODER(DEEP, bucket, flacdec::needs_wide(bps),
                  write_planar<MAXP, WIDE>(fp, flen, start, bs, skip, take, sbps, ch_tag, c, sample_format, scale,
                                           reinterpret_cast<uint32_t*>(dst), stage, ON));
}

// The zero pass of the planar form in device memory: elements [written, n_samples) of every row of every range.  Rows
// are numbered in rslot order (the ranges of c channels have c rows each); workgroup (x, y) takes rows x, x + gridDim.x,
// ... and of each row's interval the y-th share of its 16-byte vectors, lane after lane (streamplanar::split: scalar
// elements up to the first 16-byte boundary and behind the last).
__global__ void __launch_bounds__(256) ranges_zero_kernel(const Range* __restrict__ ranges,
                                                          const uint32_t* __restrict__ rperm,
                                                          const uint64_t* __restrict__ r_written, ClassLo rslot_lo,
                                                          uint32_t n_rows, uint8_t* __restrict__ out) {
  const uint32_t lane = blockIdx.y * blockDim.x + threadIdx.x, lanes = gridDim.y * blockDim.x;
  for (uint32_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    uint32_t channels = 1, row0 = 0, q0 = 0, seen = 0;
#pragma unroll
    for (uint32_t c = 1; c <= 8; ++c) {
      const uint32_t rows = c * (rslot_lo.lo[c + 1] - rslot_lo.lo[c]);
      if (row >= seen && row - seen < rows) {
        channels = c;
        row0 = seen;
        q0 = rslot_lo.lo[c];
      }
      seen += rows;
    }
    const uint32_t q = q0 + (row - row0) / channels, c = (row - row0) % channels;
    const Range& x = ranges[rperm[q]];
    const streamplanar::Interval z = streamplanar::zero_interval(r_written[q], x.n_samples);
    if (!z.count) continue;
    uint32_t* p = reinterpret_cast<uint32_t*>(out + streamplanar::element_offset(x.out_offset, x.n_samples, c, z.first));
    const streamplanar::Split s = streamplanar::split(reinterpret_cast<uintptr_t>(p), z.count);
    if (lane < s.head) p[lane] = 0u;
    uint4* body = reinterpret_cast<uint4*>(p + s.head);
    for (uint64_t v = lane; v < s.body / 4; v += lanes) body[v] = make_uint4(0u, 0u, 0u, 0u);
    if (lane < s.tail) p[s.head + s.body + lane] = 0u;
  }
}

// Both calls.  `planar`: the slots are rows of 4-byte elements in `sample_format`, else packed PCM.
int decode_ranges_call(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                       size_t n_streams, const void* ranges, size_t n_ranges, size_t max_frames, uint8_t* out,
                       uint64_t out_bytes, bool planar, uint32_t sample_format, uint64_t* totals,
                       uint64_t call_totals[2], int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const std::string who = planar ? "decode_ranges_planar" : "decode_ranges";
  uint64_t* plan = h->last_ranges_plan;  // launches, synchronisations, transfers, channel classes of the ranges
  plan[0] = plan[1] = plan[2] = plan[3] = 0;
  if (!call_limits_ok(memory_kind, n_streams, max_frames, n_bytes) || !bytes || !streams || !ranges || !out || !totals ||
      !call_totals || n_ranges > streamranges::MAX_RANGES) {
    h->last_error = who + ": null pointer, unknown memory kind, more than 2^24 streams or ranges, max_frames above "
                          "2^30 or n_bytes >= 16 TiB";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (planar && sample_format != FLACENC_HIP_SAMPLE_I32 && sample_format != FLACENC_HIP_SAMPLE_F32) {
    h->last_error = who + ": unknown sample_format";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const Desc* table = static_cast<const Desc*>(streams);
  const Range* rtable = static_cast<const Range*>(ranges);
  int rc = streamranges::check_spans(table, n_streams, n_bytes, h->max_bps);
  if (rc == FLACENC_HIP_ERR_UNSUPPORTED) {
    h->last_error = who + ": a stream's bits_per_sample not in 4..=24 (4..=32 with flacenc_hip_set_max_bits_per_sample)";
    return rc;
  }
  if (rc != FLACENC_HIP_OK) {
    h->last_error = who + ": spans not ascending, overlapping or past n_bytes, channels not in 1..=8, "
                          "max_block_size not in 1..=65536 or bytes_per_sample not in ceil(bits / 8)..=4";
    return rc;
  }
  rc = planar ? streamplanar::check_ranges(rtable, n_ranges, table, n_streams, out_bytes)
              : streamranges::check_ranges(rtable, n_ranges, table, n_streams, out_bytes);
  if (rc != FLACENC_HIP_OK) {
    h->last_error = who + ": a range's stream >= n_streams, reserved != 0, first_sample + n_samples overflows, its slot "
                          "reaches past out_bytes or (planar) its out_offset is not a multiple of 4";
    return rc;
  }
  call_totals[0] = call_totals[1] = 0;
  if (n_ranges == 0) return FLACENC_HIP_OK;
  const bool host = memory_kind == FLACENC_HIP_MEM_HOST;
  const uint32_t ns = static_cast<uint32_t>(n_streams), nr = static_cast<uint32_t>(n_ranges);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;

  // ---- the range table on its way to the device: the descriptors and the rslot order (sorted by channel count) ----
  h->ranges_table.resize(n_ranges * sizeof(Range) + n_ranges * 4);
  std::memcpy(h->ranges_table.data(), rtable, n_ranges * sizeof(Range));
  uint32_t* p_rperm = reinterpret_cast<uint32_t*>(h->ranges_table.data() + n_ranges * sizeof(Range));
  ClassLo rslot_lo{};  // rslots [lo[c], lo[c + 1]) hold the ranges on streams of c channels
  const uint32_t classes = sort_by_channels(
      n_ranges, [table, rtable](size_t r) { return table[rtable[r].stream].channels; }, rslot_lo.lo, p_rperm);

  // ---- the index; behind `base`, host memory: where[n_ranges + 1] | totals[n_ranges][4] ----
  const size_t F = max_frames;
  size_t own = 0;
  auto take = [&own](size_t bytes_) {
    const size_t at = own;
    own += a256(bytes_ + 8);
    return at;
  };
  const size_t o_ends = take(n_streams * sizeof(StreamEnd));
  const size_t o_rframes = take(n_ranges * 8), o_rbytes = take(n_ranges * 8), o_rfirst = take(n_ranges * 8);
  const size_t o_rwritten = take(n_ranges * 8), o_rbase = take((n_ranges + 1) * 8);
  const size_t o_rfrange = take(F * 4), o_rfframe = take(F * 4);
  Request rq{};
  rq.bytes = bytes;
  rq.n_bytes = n_bytes;
  rq.table = table;
  rq.n_streams = n_streams;
  rq.max_frames = max_frames;
  rq.host = host;
  rq.who = planar ? "decode_ranges_planar" : "decode_ranges";
  rq.extra_words = host ? (n_ranges + 1) + 4 * n_ranges : 0;
  rq.extra_table = h->ranges_table.data();
  rq.extra_table_bytes = h->ranges_table.size();
  rq.extra_scratch = own;
  Index ix;
  Drain drain{h};
  if ((rc = build(h, plan, rq, ix)) != FLACENC_HIP_OK) return rc;
  plan[3] = classes;
  const Range* d_ranges = reinterpret_cast<const Range*>(ix.extra_table);
  const uint32_t* rperm = reinterpret_cast<const uint32_t*>(ix.extra_table + n_ranges * sizeof(Range));
  uint64_t* where = host ? ix.extra : nullptr;
  uint64_t* d_totals = host ? ix.extra + (n_ranges + 1) : totals;
  StreamEnd* ends = reinterpret_cast<StreamEnd*>(ix.scratch + o_ends);
  uint64_t* r_frames = reinterpret_cast<uint64_t*>(ix.scratch + o_rframes);
  uint64_t* r_bytes = reinterpret_cast<uint64_t*>(ix.scratch + o_rbytes);
  uint64_t* r_first = reinterpret_cast<uint64_t*>(ix.scratch + o_rfirst);
  uint64_t* r_written = reinterpret_cast<uint64_t*>(ix.scratch + o_rwritten);
  uint64_t* r_base = reinterpret_cast<uint64_t*>(ix.scratch + o_rbase);
  uint32_t* rf_range = reinterpret_cast<uint32_t*>(ix.scratch + o_rfrange);
  uint32_t* rf_frame = reinterpret_cast<uint32_t*>(ix.scratch + o_rfframe);
  // ---- which frames every range touches ----
  COUNTED_LAUNCH(plan, ranges_streams_kernel, dim3(ceil_div(ns, 256)), dim3(256), 0, st, ix.descs, ix.perm, ns, ix.base,
                 ix.pcm, ix.bad, ix.f_node, ix.cand_pos, ix.s_end, ix.s_why, ix.counters, ends);
  if (planar)
    COUNTED_LAUNCH(plan, ranges_locate_kernel<true>, dim3(ceil_div(nr, 256)), dim3(256), 0, st, ix.descs, d_ranges, rperm,
                   nr, ends, ix.pcm, ix.f_node, ix.cand_pos, ix.counters, r_frames, r_bytes, r_first, r_written, d_totals,
                   ix.meta);
  else
    COUNTED_LAUNCH(plan, ranges_locate_kernel<false>, dim3(ceil_div(nr, 256)), dim3(256), 0, st, ix.descs, d_ranges,
                   rperm, nr, ends, ix.pcm, ix.f_node, ix.cand_pos, ix.counters, r_frames, r_bytes, r_first, r_written,
                   d_totals, ix.meta);
  HIP_TRY(h, launch_scan2(r_frames, host ? r_bytes : nullptr, nr, r_base, where, st));
  ++plan[0];
  COUNTED_LAUNCH(plan, ranges_verdict_kernel, dim3(1), dim3(1), 0, st, r_base, nr, static_cast<uint64_t>(max_frames),
                 rslot_lo, ix.counters, ix.meta);
  if (F)
    COUNTED_LAUNCH(plan, ranges_enumerate_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, st, r_base, nr, r_first,
                   ix.counters, rf_range, rf_frame);
  HIP_TRY(h, hipGetLastError());
  const uint64_t* r_meta = static_cast<const uint64_t*>(h->pin_meta[0]);
  HIP_TRY(h, hipMemcpyAsync(h->pin_meta[0], ix.meta, ix.result_words * 8, hipMemcpyDeviceToHost, st));
  ++plan[2];
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  const uint64_t* r_where = r_meta + M_WORDS + (n_streams + 1);
  const uint64_t* r_totals = r_where + (n_ranges + 1);
  if (r_meta[M_ERR]) {  // nothing reaches `out`; every range's totals are zero
    if (host) {
      std::memset(totals, 0, n_ranges * 32);
    } else {
      HIP_TRY(h, hipMemsetAsync(totals, 0, n_ranges * 32, st));
      HIP_TRY(h, hipStreamSynchronize(st));
    }
    call_totals[0] = FLACENC_HIP_INDEX_ERROR;
    drain.armed = false;
    return FLACENC_HIP_OK;
  }

  // ---- decode the ranges' frames straight into packed PCM: one launch per channel count present ----
  uint8_t* d_out = out;
  const uint64_t pcm_bytes = host ? r_where[n_ranges] : 0;
  if (host) {
    if ((rc = ensure(h, h->d_cont[0], static_cast<size_t>(pcm_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_out = static_cast<uint8_t*>(h->d_cont[0].ptr);
  }
  const bool deep = any_deep_stream(table, n_streams);
  for (uint32_t c = 1; c <= 8; ++c) {
    if (rslot_lo.lo[c] == rslot_lo.lo[c + 1]) continue;
    const uint32_t k_lo = static_cast<uint32_t>(r_meta[M_CLASS + c]), k_hi = static_cast<uint32_t>(r_meta[M_CLASS + c + 1]);
    const uint32_t per_block = 256 / c;
    // (a class whose ranges touch no frame still counts as a launch of the plan: the plan depends on the classes only)
    const dim3 grid(k_hi > k_lo ? ceil_div(k_hi - k_lo, per_block) : 1), block(per_block * c);
    if (planar && deep)
      COUNTED_LAUNCH(plan, ranges_decode_planar_kernel<true>, grid, block, 0, st, ix.d_bytes, ix.descs, d_ranges, rperm,
                     ix.base, ix.pcm, ix.f_node, ix.f_slot, rf_range, rf_frame, r_written, ix.cand_pos, ix.recs, k_lo,
                     k_hi, c, where, sample_format, d_out);
    else if (planar)
      COUNTED_LAUNCH(plan, ranges_decode_planar_kernel<false>, grid, block, 0, st, ix.d_bytes, ix.descs, d_ranges, rperm,
                     ix.base, ix.pcm, ix.f_node, ix.f_slot, rf_range, rf_frame, r_written, ix.cand_pos, ix.recs, k_lo,
                     k_hi, c, where, sample_format, d_out);
    else if (deep)
      COUNTED_LAUNCH(plan, ranges_decode_kernel<true>, grid, block, 0, st, ix.d_bytes, ix.descs, d_ranges, rperm,
                     ix.base, ix.pcm, ix.f_node, ix.f_slot, rf_range, rf_frame, r_written, ix.cand_pos, ix.recs, k_lo,
                     k_hi, c, where, d_out);
    else
      COUNTED_LAUNCH(plan, ranges_decode_kernel<false>, grid, block, 0, st, ix.d_bytes, ix.descs, d_ranges, rperm,
                     ix.base, ix.pcm, ix.f_node, ix.f_slot, rf_range, rf_frame, r_written, ix.cand_pos, ix.recs, k_lo,
                     k_hi, c, where, d_out);
  }
  if (planar && !host) {  // the rows' tails, all ranges in one launch (host memory: the host threads zero them below)
    uint64_t longest = 0;
    for (size_t r = 0; r < n_ranges; ++r) longest = std::max<uint64_t>(longest, rtable[r].n_samples);
    uint32_t n_rows = 0;
    for (uint32_t c = 1; c <= 8; ++c) n_rows += c * (rslot_lo.lo[c + 1] - rslot_lo.lo[c]);
    // a share of 4096 vectors (16 per lane) of the longest row per workgroup, 64 shares at the most
    const uint32_t shares = static_cast<uint32_t>(std::min<uint64_t>(64, std::max<uint64_t>(1, (longest + 16383) / 16384)));
    COUNTED_LAUNCH(plan, ranges_zero_kernel, dim3(std::min<uint32_t>(n_rows, 32768), shares), dim3(256), 0, st, d_ranges,
                   rperm, r_written, rslot_lo, n_rows, d_out);
  }
  HIP_TRY(h, hipGetLastError());
  // host memory: one transfer of the ranges' PCM back to back into pinned staging, then every range to its slot
  if (host && (rc = download_pcm(h, plan, rq.who, d_out, pcm_bytes)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  drain.armed = false;
  if (host) {
    const uint8_t* staged = static_cast<const uint8_t*>(h->pin_out[0]);
    for (size_t q = 0; q < n_ranges; ++q) {
      const uint64_t n = r_where[q + 1] - r_where[q];
      const Range& x = rtable[p_rperm[q]];
      if (!planar) {
        if (n) h->copy_pool->copy(out + x.out_offset, staged + r_where[q], static_cast<size_t>(n));
        continue;
      }
      // staged: the range's rows of `written` elements back to back; each to the front of its row of the slot, zeros
      // behind it
      const uint32_t channels = table[x.stream].channels;
      const uint64_t written = n / (static_cast<uint64_t>(channels) * streamplanar::ELEM);
      const streamplanar::Interval z = streamplanar::zero_interval(written, x.n_samples);
      for (uint32_t c = 0; c < channels; ++c) {
        uint8_t* row = out + streamplanar::element_offset(x.out_offset, x.n_samples, c, 0);
        if (written)
          h->copy_pool->copy(row, staged + streamplanar::element_offset(r_where[q], written, c, 0),
                             static_cast<size_t>(written * streamplanar::ELEM));
        if (z.count) std::memset(row + z.first * streamplanar::ELEM, 0, static_cast<size_t>(z.count * streamplanar::ELEM));
      }
    }
    std::memcpy(totals, r_totals, n_ranges * 32);
  }
  call_totals[0] = r_meta[M_FRAMES];
  call_totals[1] = r_meta[M_SAMPLES];
  return FLACENC_HIP_OK;
}

}  // namespace
}  // namespace flacenc_hip

extern "C" int flacenc_hip_decode_ranges(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                         const void* streams, size_t n_streams, const void* ranges, size_t n_ranges,
                                         size_t max_frames, uint8_t* out, uint64_t out_bytes, uint64_t* totals,
                                         uint64_t call_totals[2], int memory_kind) {
  return flacenc_hip::decode_ranges_call(h, bytes, n_bytes, streams, n_streams, ranges, n_ranges, max_frames, out,
                                         out_bytes, false, 0, totals, call_totals, memory_kind);
}

extern "C" int flacenc_hip_decode_ranges_planar(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                                const void* streams, size_t n_streams, const void* ranges,
                                                size_t n_ranges, size_t max_frames, void* out, uint64_t out_bytes,
                                                uint32_t sample_format, uint64_t* totals, uint64_t call_totals[2],
                                                int memory_kind) {
  return flacenc_hip::decode_ranges_call(h, bytes, n_bytes, streams, n_streams, ranges, n_ranges, max_frames,
                                         static_cast<uint8_t*>(out), out_bytes, true, sample_format, totals, call_totals,
                                         memory_kind);
}
