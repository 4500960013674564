// flac_decode_streams.cpp -- flacenc_hip_decode_streams: a batch of FLAC streams to packed PCM in one call, with a number
// of launches, synchronisations and transfers that does not depend on the number of streams.
//
// The index -- every stream's verified chain, every chain frame enumerated in `slot` order (the table sorted by channel
// count, so that the frames of one channel count are one range) and the two scans over the frame sequence (PCM bytes,
// frames with a status) -- is streamindex::build (stream_index.h, stream_index.cpp), which flacenc_hip_decode_ranges
// (flac_decode_ranges.cpp) runs too.  This file holds what follows it:
//   streams_totals_kernel  the cut: one lane per stream bisects for the first frame that has a status or no longer fits
//                          its slot (stream_batch_core.h)
//   streams_decode_kernel  reconstruction from the index's own skim records -- no second skim or CRC of a frame -- with
//                          one launch per channel count present and the lane rules of subframe_kernel: a frame's channels
//                          on adjacent lanes of one workgroup, a stereo pair on an even / odd lane pair, a wave at its
//                          largest order bucket.  A lane writes its channel's samples straight into the packed interleaved
//                          little-endian PCM (the flacenc_hip_pack_le_bytes layout) at the frame's own destination,
//                          channel count and width: no intermediate rows (write_pcm, flac_decode_device.h)
// flacenc_hip_decode_streams_md5 is the same call with one more step behind the decode launches: one lane per stream
// hashes the bytes the stream's lanes just wrote (md5_streams.cpp), on the device, before the PCM is downloaded.
#include "api_internal.h"
#include "flac_decode_device.h"
#include "md5_core.h"
#include "stream_batch_core.h"
#include "stream_index.h"

namespace flacenc_hip {
namespace {

using namespace streamindex;  // the counters' and meta words' names, Request / Index, Drain

using flacdec::FrameRec;
using Desc = flacenc_hip_stream_desc;

// one lane per slot: the cut, the stream's totals and what the call adds up
__global__ void __launch_bounds__(256) streams_totals_kernel(const Desc* __restrict__ descs,
                                                             const uint32_t* __restrict__ perm, uint32_t n_streams,
                                                             const uint64_t* __restrict__ base,
                                                             const uint64_t* __restrict__ pcm,
                                                             const uint64_t* __restrict__ bad,
                                                             const uint32_t* __restrict__ f_node,
                                                             const uint64_t* __restrict__ cand_pos,
                                                             const uint64_t* __restrict__ s_end,
                                                             const uint32_t* __restrict__ s_why,
                                                             const uint32_t* __restrict__ counters,
                                                             uint32_t* __restrict__ s_accepted,
                                                             uint64_t* __restrict__ s_bytes, uint64_t* __restrict__ totals,
                                                             uint64_t* __restrict__ meta) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const uint32_t s = perm[i];
  uint64_t frames = 0, samples = 0, consumed = 0, why = 0, bytes = 0;
  if (!counters[C_ERR]) {
    const Desc& d = descs[s];
    const uint64_t first = base[i], count = base[i + 1] - first;
    frames = streambatch::accepted_frames(pcm, bad, first, count, d.out_capacity);
    bytes = pcm[first + frames] - pcm[first];
    samples = bytes / (static_cast<uint64_t>(d.channels) * d.bytes_per_sample);
    if (frames < count) {  // stopped at a frame of the chain: its own status first, as flacenc_hip_decode_pcm
      const uint64_t m = first + frames;
      consumed = cand_pos[f_node[m]] - d.offset;
      why = bad[m + 1] != bad[m] ? FLACENC_HIP_DECODE_UNSUPPORTED : FLACENC_HIP_DECODE_NO_ROOM;
    } else {
      consumed = s_end[s] - d.offset;
      why = s_why[s];
    }
    if (frames) {
      atomicAdd(reinterpret_cast<unsigned long long*>(meta + M_FRAMES), static_cast<unsigned long long>(frames));
      atomicAdd(reinterpret_cast<unsigned long long*>(meta + M_SAMPLES), static_cast<unsigned long long>(samples));
    }
  }
  s_accepted[i] = static_cast<uint32_t>(frames);
  s_bytes[s] = bytes;
  totals[4 * static_cast<size_t>(s) + 0] = frames;
  totals[4 * static_cast<size_t>(s) + 1] = samples;
  totals[4 * static_cast<size_t>(s) + 2] = consumed;
  totals[4 * static_cast<size_t>(s) + 3] = why;
}

// The frames [m_lo, m_hi) of the sequence all have `channels` channels; lane (frame, c) as in subframe_kernel.  A frame
// behind its stream's cut keeps its lanes idle.  A stream's PCM starts at out + where[stream] (`where` given: the
// compact staging of the host path) or at out + its out_offset.  DEEP: see AT_WAVE_DECODER.
template <bool DEEP>
__global__ void __launch_bounds__(256) streams_decode_kernel(const uint8_t* __restrict__ bytes,
                                                             const Desc* __restrict__ descs,
                                                             const uint32_t* __restrict__ perm,
                                                             const uint64_t* __restrict__ base,
                                                             const uint64_t* __restrict__ pcm,
                                                             const uint32_t* __restrict__ f_node,
                                                             const uint32_t* __restrict__ f_slot,
                                                             const uint32_t* __restrict__ s_accepted,
                                                             const uint64_t* __restrict__ cand_pos,
                                                             const FrameRec* __restrict__ recs, uint32_t m_lo,
                                                             uint32_t m_hi, uint32_t channels,
                                                             const uint64_t* __restrict__ where, uint8_t* __restrict__ out) {
  const uint32_t per_block = blockDim.x / channels;  // frames never straddle workgroups
  const uint32_t lf = threadIdx.x / channels, c = threadIdx.x % channels;
  const uint64_t m = static_cast<uint64_t>(m_lo) + static_cast<uint64_t>(blockIdx.x) * per_block + lf;
  uint32_t bs = 0, ch_tag = 0, flen = 0, start = 0, bps = 0, B = 1;
  const uint8_t* fp = bytes;
  uint8_t* dst = out;
  if (lf < per_block && m < m_hi) {
    const uint32_t i = f_slot[m], s = perm[i];
    if (m - base[i] < s_accepted[i]) {
      const Desc& d = descs[s];
      const uint32_t node = f_node[m];
      const FrameRec& r = recs[node];
      bs = r.block_size;
      ch_tag = (r.info >> 4) & 15u;
      flen = r.len;
      start = r.sub_bit[c];
      bps = d.bits_per_sample;
      B = d.bytes_per_sample;
      fp = bytes + cand_pos[node];
      dst = out + (where ? where[s] : d.out_offset) + (pcm[m] - pcm[base[i]]);
    }
  }
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const int bucket = lane_bucket(fp, flen, start, bs, sbps);
  AT_WAVE_DECODER(DEEP, bucket, flacdec::needs_wide(bps),
                  write_pcm<MAXP, WIDE>(fp, flen, start, bs, 0, bs, sbps, ch_tag, c, channels, B, dst, ON));
}

// the digest of the empty string, for the streams of a call that wrote nothing
void empty_digests(uint8_t* digests, size_t n) {
  uint8_t d[16];
  md5core::md5_bytes(nullptr, 0, d);
  for (size_t s = 0; s < n; ++s) std::memcpy(digests + 16 * s, d, 16);
}

// flacenc_hip_decode_streams (md5 false: `digests` is not looked at, and the plan is the one that call has always had)
// and flacenc_hip_decode_streams_md5: the same call, plus one lane per stream that hashes what the stream's lanes wrote
// -- behind the decode launches, in front of the download, on the device copy of the PCM.
int decode_streams_impl(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                        size_t n_streams, size_t max_frames, uint8_t* out, uint64_t out_bytes, uint64_t* totals,
                        uint64_t call_totals[2], int memory_kind, bool md5, uint8_t* digests) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  uint64_t* plan = h->last_streams_plan;  // launches, synchronisations, transfers, channel classes
  plan[0] = plan[1] = plan[2] = plan[3] = 0;
  if (!call_limits_ok(memory_kind, n_streams, max_frames, n_bytes) || !bytes || !streams || !out || !totals ||
      !call_totals || (md5 && !digests)) {
    h->last_error = "decode_streams: null pointer, unknown memory kind, more than 2^24 streams, max_frames above 2^30 or "
                    "n_bytes >= 16 TiB";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const Desc* table = static_cast<const Desc*>(streams);
  int rc = streambatch::check_streams(table, n_streams, n_bytes, out_bytes, h->max_bps);
  if (rc == FLACENC_HIP_ERR_UNSUPPORTED) {
    h->last_error = "decode_streams: a stream's bits_per_sample not in 4..=24 (4..=32 with "
                    "flacenc_hip_set_max_bits_per_sample)";
    return rc;
  }
  if (rc != FLACENC_HIP_OK) {
    h->last_error = "decode_streams: spans not ascending, overlapping or past n_bytes, a slot past out_bytes, channels "
                    "not in 1..=8, max_block_size not in 1..=65536 or bytes_per_sample not in ceil(bits / 8)..=4";
    return rc;
  }
  call_totals[0] = call_totals[1] = 0;
  if (n_streams == 0) return FLACENC_HIP_OK;
  const bool host = memory_kind == FLACENC_HIP_MEM_HOST;
  const uint32_t ns = static_cast<uint32_t>(n_streams);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;

  // ---- the segmented index (stream_index.h); behind `base`, host memory: totals | where ----
  Request rq{};
  rq.bytes = bytes;
  rq.n_bytes = n_bytes;
  rq.table = table;
  rq.n_streams = n_streams;
  rq.max_frames = max_frames;
  rq.host = host;
  rq.who = "decode_streams";
  rq.extra_words = host ? 4 * n_streams + (n_streams + 1) : 0;
  // (host memory, md5: the digests come down into the same pinned slot, behind the results)
  rq.pinned_tail = host && md5 ? n_streams * 16 : 0;
  rq.extra_scratch = host && md5 ? n_streams * 16 : 0;
  Index ix;
  Drain drain{h};
  if ((rc = build(h, plan, rq, ix)) != FLACENC_HIP_OK) return rc;
  const size_t result_words = ix.result_words;
  uint64_t* d_totals = host ? ix.extra : totals;
  uint64_t* where = host ? ix.extra + 4 * n_streams : nullptr;
  uint8_t* d_digests = host ? reinterpret_cast<uint8_t*>(ix.scratch) : digests;
  // ---- the cut ----
  COUNTED_LAUNCH(plan, streams_totals_kernel, dim3(ceil_div(ns, 256)), dim3(256), 0, st, ix.descs, ix.perm, ns, ix.base,
                 ix.pcm, ix.bad, ix.f_node, ix.cand_pos, ix.s_end, ix.s_why, ix.counters, ix.s_accepted, ix.s_bytes,
                 d_totals, ix.meta);
  if (host) {
    HIP_TRY(h, launch_scan2(ix.s_bytes, nullptr, ns, where, nullptr, st));
    ++plan[0];
  }
  // device memory: should the call end with INDEX_ERROR, every digest is the empty string's.  Written now, in front of
  // the one synchronisation that path has; the launch behind the decode overwrites it.  (Host memory: the host writes.)
  if (md5 && !host) {
    HIP_TRY(h, launch_md5_spans(ix.d_bytes, nullptr, 0, nullptr, nullptr, ns, d_digests, st));
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
  const uint64_t* r_where = r_totals + 4 * n_streams;
  if (r_meta[M_ERR]) {  // nothing reaches `out`; every stream's totals are zero (the kernel wrote them so)
    if (host) std::memcpy(totals, r_totals, n_streams * 32);
    if (host && md5) empty_digests(digests, n_streams);
    call_totals[0] = FLACENC_HIP_INDEX_ERROR;
    drain.armed = false;
    return FLACENC_HIP_OK;
  }

  // ---- decode straight into packed PCM: one launch per channel count present ----
  uint8_t* d_out = out;
  const bool deep = any_deep_stream(table, n_streams);
  const uint64_t pcm_bytes = host ? r_where[n_streams] : 0;
  if (host) {
    if ((rc = ensure(h, h->d_cont[0], static_cast<size_t>(pcm_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_out = static_cast<uint8_t*>(h->d_cont[0].ptr);
  }
  for (uint32_t c = 1; c <= 8; ++c) {
    if (ix.slot_lo[c] == ix.slot_lo[c + 1]) continue;
    const uint32_t m_lo = static_cast<uint32_t>(r_base[ix.slot_lo[c]]), m_hi = static_cast<uint32_t>(r_base[ix.slot_lo[c + 1]]);
    const uint32_t per_block = 256 / c;
    // (a class whose streams hold no frame still counts as a launch of the plan: the plan depends on the classes only)
    const dim3 grid(m_hi > m_lo ? ceil_div(m_hi - m_lo, per_block) : 1), block(per_block * c);
    if (deep)
      COUNTED_LAUNCH(plan, streams_decode_kernel<true>, grid, block, 0, st, ix.d_bytes, ix.descs, ix.perm, ix.base,
                     ix.pcm, ix.f_node, ix.f_slot, ix.s_accepted, ix.cand_pos, ix.recs, m_lo, m_hi, c, where, d_out);
    else
      COUNTED_LAUNCH(plan, streams_decode_kernel<false>, grid, block, 0, st, ix.d_bytes, ix.descs, ix.perm, ix.base,
                     ix.pcm, ix.f_node, ix.f_slot, ix.s_accepted, ix.cand_pos, ix.recs, m_lo, m_hi, c, where, d_out);
  }
  HIP_TRY(h, hipGetLastError());
  if (md5) {
    // stream s wrote s_bytes[s] bytes from d_out + where[s] (the compact staging) resp. + its out_offset, the third of
    // the descriptor's six words
    const uint64_t* first = where ? where : reinterpret_cast<const uint64_t*>(ix.descs) + 2;
    HIP_TRY(h, launch_md5_spans(d_out, first, where ? 1u : static_cast<uint32_t>(sizeof(Desc) / 8), ix.s_bytes, nullptr,
                                ns, d_digests, st));
    ++plan[0];
    if (host) {
      HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(h->pin_meta[0]) + result_words * 8, d_digests, n_streams * 16,
                                hipMemcpyDeviceToHost, st));
      ++plan[2];
    }
  }
  // host memory: one transfer of the streams' PCM back to back into pinned staging, then every stream to its slot
  if (host && (rc = download_pcm(h, plan, "decode_streams", d_out, pcm_bytes)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipStreamSynchronize(st));
  ++plan[1];
  drain.armed = false;
  if (host) {
    const uint8_t* staged = static_cast<const uint8_t*>(h->pin_out[0]);
    for (size_t s = 0; s < n_streams; ++s) {
      const uint64_t n = r_where[s + 1] - r_where[s];
      if (n) h->copy_pool->copy(out + table[s].out_offset, staged + r_where[s], static_cast<size_t>(n));
    }
    std::memcpy(totals, r_totals, n_streams * 32);
    if (md5) std::memcpy(digests, static_cast<const char*>(h->pin_meta[0]) + result_words * 8, n_streams * 16);
  }
  call_totals[0] = r_meta[M_FRAMES];
  call_totals[1] = r_meta[M_SAMPLES];
  return FLACENC_HIP_OK;
}

}  // namespace
}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" int flacenc_hip_decode_streams(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                          const void* streams, size_t n_streams, size_t max_frames, uint8_t* out,
                                          uint64_t out_bytes, uint64_t* totals, uint64_t call_totals[2],
                                          int memory_kind) {
  return decode_streams_impl(h, bytes, n_bytes, streams, n_streams, max_frames, out, out_bytes, totals, call_totals,
                             memory_kind, false, nullptr);
}

extern "C" int flacenc_hip_decode_streams_md5(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                              const void* streams, size_t n_streams, size_t max_frames, uint8_t* out,
                                              uint64_t out_bytes, uint64_t* totals, uint64_t call_totals[2],
                                              int memory_kind, uint8_t* digests) {
  return decode_streams_impl(h, bytes, n_bytes, streams, n_streams, max_frames, out, out_bytes, totals, call_totals,
                             memory_kind, true, digests);
}
