// flac_decode_streams.cpp -- flacenc_hip_decode_streams: a batch of FLAC streams to packed PCM in one call, with a number
// of launches, synchronisations and transfers that does not depend on the number of streams.
//
// The index of flac_decode.cpp, segmented: a byte position is a candidate only inside a stream's span and its header is
// judged with that stream's parameters; skim and CRC-16 run per candidate, bounded by the stream's end; links stay
// inside a stream ("ends at the stream's end" is the end sentinel); every stream has its own chain root, the verified
// candidate at its first byte.  One lane per stream measures its chain by binary lifting over the jump levels, a scan
// over streams gives frame bases, and every frame of every stream is enumerated by its own lane.  Streams are numbered
// in `slot` order -- the table sorted by channel count -- so that the frames of one channel count are one range.
// The cut: two scans over the frame sequence (PCM bytes, frames with a status) and one lane per stream that bisects for
// the first frame that has a status or no longer fits its slot (stream_batch_core.h).
// Reconstruction starts from the index's own skim records -- no second skim or CRC of a frame -- with one launch per
// channel count present and the lane rules of subframe_kernel: a frame's channels on adjacent lanes of one workgroup,
// a stereo pair on an even / odd lane pair, a wave at its largest order bucket.  A lane writes its channel's samples
// straight into the packed interleaved little-endian PCM (the flacenc_hip_pack_le_bytes layout) at the frame's own
// destination, channel count and width: no intermediate rows.
// flacenc_hip_decode_streams_md5 is the same call with one more step behind the decode launches: one lane per stream
// hashes the bytes the stream's lanes just wrote (md5_streams.cpp), on the device, before the PCM is downloaded.
// The index -- everything up to the two scans over the frame sequence -- is streamindex::build (stream_index.h), which
// flacenc_hip_decode_ranges (flac_decode_ranges.cpp) runs too; its kernels live here.
#include "api_internal.h"
#include "flac_decode.h"
#include "flac_decode_core.h"
#include "md5_core.h"
#include "stream_batch_core.h"
#include "stream_index.h"

namespace flacenc_hip {
namespace {

using namespace streamindex;  // the counters' and meta words' names, Request / Index, Drain

using flacdec::FrameRec;
using Desc = flacenc_hip_stream_desc;

__constant__ flacdec::CrcTables kCrc = flacdec::make_crc_tables();

constexpr uint32_t kEnd = 0xFFFFFFFEu, kDead = 0xFFFFFFFFu;  // chain sentinels, as in flac_decode.cpp
constexpr uint32_t kPosPerThread = 16, kPosPerBlock = 256 * kPosPerThread;

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

// ---------------------------------------------------------------- candidates
// the stream for which byte p starts a valid header, NONE otherwise; the table is consulted only behind the sync test
__device__ uint32_t candidate_stream(const uint8_t* bytes, uint64_t n_bytes, const Desc* descs, uint32_t n_streams,
                                     uint64_t p) {
  if (p + 1 >= n_bytes || bytes[p] != 0xFFu || (bytes[p + 1] & 0xFEu) != 0xF8u) return streambatch::NONE;
  const uint32_t s = streambatch::stream_of_byte(descs, n_streams, p);
  if (s == streambatch::NONE) return s;
  const uint64_t left = descs[s].offset + descs[s].n_bytes - p;  // what the parse may read ends with the stream
  flacdec::Header h;
  return flacdec::parse_header(bytes + p, left > 64 ? 64u : static_cast<uint32_t>(left), descs[s].channels,
                               descs[s].bits_per_sample, 65536u, kCrc, h) == 0
             ? s
             : streambatch::NONE;
}

// exclusive scan of v over the workgroup (256 threads); returns the exclusive prefix, *total = the sum
__device__ uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
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

// WRITE false: block_counts[block] = its candidates.  WRITE true: block_offsets (their exclusive scan) in, the
// candidates' positions and streams out in ascending order, and the total in counters[C_CANDS]
template <bool WRITE>
__global__ void __launch_bounds__(256) streams_cand_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                           const Desc* __restrict__ descs, uint32_t n_streams,
                                                           uint64_t* __restrict__ block_counts,
                                                           const uint64_t* __restrict__ block_offsets,
                                                           uint64_t* __restrict__ cand_pos,
                                                           uint32_t* __restrict__ cand_stream, uint32_t capacity,
                                                           uint32_t* __restrict__ counters) {
  __shared__ uint32_t sh[256];
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock + threadIdx.x * kPosPerThread;
  uint32_t mask = 0;
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if (candidate_stream(bytes, n_bytes, descs, n_streams, base + k) != streambatch::NONE) mask |= 1u << k;
  uint32_t total;
  const uint32_t before = block_scan(__popc(mask), sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
    return;
  }
  uint64_t at = block_offsets[blockIdx.x] + before;
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if ((mask >> k) & 1u) {
      if (at < capacity) {
        cand_pos[at] = base + k;
        cand_stream[at] = streambatch::stream_of_byte(descs, n_streams, base + k);
      }
      ++at;
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t all = block_offsets[gridDim.x];
    counters[C_CANDS] = all > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(all);
  }
}

// Exclusive prefix sums of up to two arrays (b may be null) by one workgroup that walks them 1024 at a time and carries
// the running sum, pcm_offsets_kernel's scan: out[i] = the sum of in[perm ? perm[j] : j] over j < i, out[n] the total.
// n = min(n_host, *n_dev) when n_dev is given.
__global__ void __launch_bounds__(1024) streams_scan_kernel(const uint64_t* __restrict__ a,
                                                            const uint64_t* __restrict__ b,
                                                            const uint32_t* __restrict__ perm, uint64_t n_host,
                                                            const uint32_t* __restrict__ n_dev,
                                                            uint64_t* __restrict__ out_a, uint64_t* __restrict__ out_b) {
  __shared__ unsigned long long wave_sums[16];
  __shared__ unsigned long long carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t n = n_host;
  if (n_dev && *n_dev < n) n = *n_dev;
  for (int which = 0; which < 2; ++which) {
    const uint64_t* in = which ? b : a;
    uint64_t* out = which ? out_b : out_a;
    if (!in) continue;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < n; base += 1024u) {
      const uint64_t i = base + tid;
      unsigned long long v = 0;
      if (i < n) v = in[perm ? perm[i] : i];
      unsigned long long s = v;  // inclusive scan inside the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(s, d, 64);
        if (static_cast<int>(lane) >= d) s += o;
      }
      if (lane == 63) wave_sums[wave] = s;
      __syncthreads();
      unsigned long long before = carry;
      for (uint32_t w = 0; w < wave; ++w) before += wave_sums[w];
      if (i < n) out[i] = before + s - v;
      __syncthreads();
      if (tid == 1023) carry = before + s;
      __syncthreads();
    }
    if (tid == 0) out[n] = carry;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- skim and link, per candidate with its stream
__global__ void __launch_bounds__(256) streams_skim_kernel(const uint8_t* __restrict__ bytes,
                                                           const Desc* __restrict__ descs,
                                                           const uint64_t* __restrict__ cand_pos,
                                                           const uint32_t* __restrict__ cand_stream,
                                                           const uint32_t* __restrict__ counters, uint32_t capacity,
                                                           FrameRec* __restrict__ recs) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Desc& d = descs[cand_stream[i]];
  const uint64_t off = cand_pos[i], left = d.offset + d.n_bytes - off;  // a candidate lies inside its stream
  FrameRec rec;
  flacdec::skim_frame(bytes + off, left > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(left), d.channels,
                      d.bits_per_sample, 65536u, false, kCrc, rec, nullptr);
  recs[i] = rec;
}

// jump[0][i]: the verified candidate that starts where candidate i ends, kEnd at its stream's end, kDead otherwise.  A
// frame ends inside its stream and spans do not overlap, so the candidate found there belongs to the same stream.
__global__ void __launch_bounds__(256) streams_link_kernel(const Desc* __restrict__ descs,
                                                           const uint64_t* __restrict__ cand_pos,
                                                           const uint32_t* __restrict__ cand_stream,
                                                           const FrameRec* __restrict__ recs,
                                                           const uint32_t* __restrict__ counters, uint32_t capacity,
                                                           uint32_t* __restrict__ jump) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = kDead;
  if (recs[i].status == 0) {
    const Desc& d = descs[cand_stream[i]];
    const uint64_t e = cand_pos[i] + recs[i].len;
    if (e == d.offset + d.n_bytes) {
      nx = kEnd;
    } else {
      uint32_t lo = i + 1, hi = n;  // positions ascend
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cand_pos[mid] < e) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n && cand_pos[lo] == e && recs[lo].status == 0) nx = lo;
    }
  }
  jump[i] = nx;
}

// ---------------------------------------------------------------- chains: one lane per stream
__global__ void __launch_bounds__(256) streams_chain_kernel(const Desc* __restrict__ descs, uint32_t n_streams,
                                                            const uint64_t* __restrict__ cand_pos,
                                                            const FrameRec* __restrict__ recs,
                                                            const uint32_t* __restrict__ jump, uint32_t levels,
                                                            const uint32_t* __restrict__ counters, uint32_t capacity,
                                                            uint64_t* __restrict__ s_frames, uint32_t* __restrict__ s_root,
                                                            uint64_t* __restrict__ s_end, uint32_t* __restrict__ s_why) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  const Desc& d = descs[s];
  const uint32_t n = min(counters[C_CANDS], capacity);
  uint64_t count = 0, end = d.offset;
  uint32_t root = kDead, why = 0;
  if (d.n_bytes != 0) {
    uint32_t lo = 0, hi = n;  // the root: the verified candidate at the stream's first byte
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (cand_pos[mid] < d.offset) lo = mid + 1;
      else hi = mid;
    }
    if (lo < n && cand_pos[lo] == d.offset && recs[lo].status == 0) root = lo;
    if (root == kDead) {
      why = FLACENC_HIP_DECODE_CHAIN;
    } else {
      uint32_t cur = root;
      count = 1;
      for (int k = static_cast<int>(levels) - 1; k >= 0; --k) {
        const uint32_t nx = jump[static_cast<size_t>(k) * capacity + cur];
        if (nx < kEnd) {
          cur = nx;
          count += 1ull << k;
        }
      }
      end = cand_pos[cur] + recs[cur].len;
      if (jump[cur] != kEnd) why = FLACENC_HIP_DECODE_CHAIN;
    }
  }
  s_frames[s] = count;
  s_root[s] = root;
  s_end[s] = end;
  s_why[s] = why;
}

// one thread: more chain frames than max_frames or more candidates than the table holds end the call with the flag
__global__ void streams_verdict_kernel(const uint64_t* __restrict__ base, uint32_t n_streams, uint64_t max_frames,
                                       uint32_t capacity, uint32_t* __restrict__ counters, uint64_t* __restrict__ meta) {
  const uint64_t total = base[n_streams];
  const uint32_t err = counters[C_CANDS] > capacity || total > max_frames;
  counters[C_ERR] = err;
  counters[C_FRAMES] = err ? 0u : static_cast<uint32_t>(total);
  meta[M_ERR] = err;
  meta[M_CHAIN] = total;
  meta[M_CANDS] = counters[C_CANDS];
}

// frame m of the sequence: its slot, its candidate (the m - base[slot]-th of the stream's chain), the PCM bytes it
// decodes to and whether it has a status (a block above the stream's max_block_size: the one status a verified frame
// can still get)
__global__ void __launch_bounds__(256) streams_enumerate_kernel(const Desc* __restrict__ descs,
                                                                const uint32_t* __restrict__ perm, uint32_t n_streams,
                                                                const uint64_t* __restrict__ base,
                                                                const uint32_t* __restrict__ s_root,
                                                                const FrameRec* __restrict__ recs,
                                                                const uint32_t* __restrict__ jump, uint32_t levels,
                                                                const uint32_t* __restrict__ counters, uint32_t capacity,
                                                                uint32_t* __restrict__ f_node, uint32_t* __restrict__ f_slot,
                                                                uint64_t* __restrict__ f_pcm, uint64_t* __restrict__ f_bad) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= counters[C_FRAMES]) return;
  const uint32_t i = streambatch::slot_of_frame(base, n_streams, m), s = perm[i];
  const uint32_t j = m - static_cast<uint32_t>(base[i]);
  uint32_t node = s_root[s];
  for (uint32_t k = 0; k < levels; ++k)
    if ((j >> k) & 1u) node = jump[static_cast<size_t>(k) * capacity + node];
  const Desc& d = descs[s];
  const uint32_t bs = recs[node].block_size;
  f_node[m] = node;
  f_slot[m] = i;
  f_pcm[m] = static_cast<uint64_t>(bs) * d.channels * d.bytes_per_sample;
  f_bad[m] = bs > d.max_block_size ? 1u : 0u;
}

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

// ---------------------------------------------------------------- reconstruction: one lane per subframe
// `bs` samples of channel c into the frame's packed PCM at dst: sample t at dst + (t * channels + c) * B, the low B
// bytes of its value, little-endian.  Whole samples where the address allows, else bytes: a neighbouring sample's bytes
// are another lane's and are never read back.
template <int MAXP>
__device__ void decode_subframe(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t sbps,
                                uint32_t ch_tag, uint32_t c, uint32_t channels, uint32_t B, uint8_t* dst) {
  flacdec::SubDecoder<MAXP> d;
  if (bs) d.init(fp, flen, start, bs, sbps);
  const bool stereo = ch_tag >= 8;
  uint8_t* p = dst + static_cast<size_t>(c) * B;
  const size_t step = static_cast<size_t>(channels) * B;
  const bool whole = (B == 2 || B == 4) && (reinterpret_cast<uintptr_t>(p) & (B - 1)) == 0;
  for (uint32_t t = 0; t < bs; ++t) {
    int32_t v = d.next();
    if (stereo) {
      const int32_t o = __shfl_xor(v, 1);
      int32_t a = c == 0 ? v : o, b = c == 0 ? o : v;
      flacdec::undo_stereo(ch_tag, a, b);
      v = c == 0 ? a : b;
    }
    const uint32_t u = static_cast<uint32_t>(v);
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

// The frames [m_lo, m_hi) of the sequence all have `channels` channels; lane (frame, c) as in subframe_kernel.  A frame
// behind its stream's cut keeps its lanes idle.  A stream's PCM starts at out + where[stream] (`where` given: the
// compact staging of the host path) or at out + its out_offset.
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
  uint32_t order = 0;
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  if (bs) {
    flacdec::BitReader r;
    r.init(fp, flen, start);
    flacdec::SubInfo si;
    flacdec::parse_subframe_header(r, bs, sbps, si);
    order = si.order;
  }
  const int bucket = flacdec::order_bucket(order);
  if (__any(bucket == 32)) decode_subframe<32>(fp, flen, start, bs, sbps, ch_tag, c, channels, B, dst);
  else if (__any(bucket == 16)) decode_subframe<16>(fp, flen, start, bs, sbps, ch_tag, c, channels, B, dst);
  else if (__any(bucket == 8)) decode_subframe<8>(fp, flen, start, bs, sbps, ch_tag, c, channels, B, dst);
  else decode_subframe<4>(fp, flen, start, bs, sbps, ch_tag, c, channels, B, dst);
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
  if ((memory_kind != FLACENC_HIP_MEM_HOST && memory_kind != FLACENC_HIP_MEM_DEVICE) || !bytes || !streams || !out ||
      !totals || !call_totals || (md5 && !digests) || n_streams > streambatch::MAX_STREAMS ||
      max_frames > streambatch::MAX_FRAMES ||
      n_bytes > (static_cast<uint64_t>(0xFFFFFFFFu) << 12)) {
    h->last_error = "decode_streams: null pointer, unknown memory kind, more than 2^24 streams, max_frames above 2^30 or "
                    "n_bytes >= 16 TiB";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const Desc* table = static_cast<const Desc*>(streams);
  int rc = streambatch::check_streams(table, n_streams, n_bytes, out_bytes);
  if (rc == FLACENC_HIP_ERR_UNSUPPORTED) {
    h->last_error = "decode_streams: a stream's bits_per_sample not in 4..=24";
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
  uint32_t* counters = ix.counters;
  uint64_t *meta = ix.meta, *base = ix.base;
  uint64_t* d_totals = host ? ix.extra : totals;
  uint64_t* where = host ? ix.extra + 4 * n_streams : nullptr;
  const Desc* descs = ix.descs;
  const uint32_t* perm = ix.perm;
  const uint32_t* slot_lo = ix.slot_lo;
  const uint8_t* d_bytes = ix.d_bytes;
  uint64_t *cand_pos = ix.cand_pos, *s_end = ix.s_end, *s_bytes = ix.s_bytes, *pcm = ix.pcm, *bad = ix.bad;
  FrameRec* recs = ix.recs;
  uint32_t *s_why = ix.s_why, *s_accepted = ix.s_accepted, *f_node = ix.f_node, *f_slot = ix.f_slot;
  uint8_t* d_digests = host ? reinterpret_cast<uint8_t*>(ix.scratch) : digests;
#define SB_LAUNCH(...)                 \
  do {                                 \
    hipLaunchKernelGGL(__VA_ARGS__);   \
    ++plan[0];                         \
  } while (0)
  // ---- the cut ----
  SB_LAUNCH(streams_totals_kernel, dim3(ceil_div(ns, 256)), dim3(256), 0, st, descs, perm, ns, base, pcm, bad, f_node,
            cand_pos, s_end, s_why, counters, s_accepted, s_bytes, d_totals, meta);
  if (host)
    SB_LAUNCH(streams_scan_kernel, dim3(1), dim3(1024), 0, st, s_bytes, nullptr, nullptr, static_cast<uint64_t>(ns),
              nullptr, where, nullptr);
  // device memory: should the call end with INDEX_ERROR, every digest is the empty string's.  Written now, in front of
  // the one synchronisation that path has; the launch behind the decode overwrites it.  (Host memory: the host writes.)
  if (md5 && !host) {
    HIP_TRY(h, launch_md5_spans(d_bytes, nullptr, 0, nullptr, nullptr, ns, d_digests, st));
    ++plan[0];
  }
  HIP_TRY(h, hipGetLastError());
  const uint64_t* r_meta = static_cast<const uint64_t*>(h->pin_meta[0]);
  HIP_TRY(h, hipMemcpyAsync(h->pin_meta[0], meta, result_words * 8, hipMemcpyDeviceToHost, st));
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
  const uint64_t pcm_bytes = host ? r_where[n_streams] : 0;
  if (host) {
    if ((rc = ensure(h, h->d_cont[0], static_cast<size_t>(pcm_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_out = static_cast<uint8_t*>(h->d_cont[0].ptr);
  }
  for (uint32_t c = 1; c <= 8; ++c) {
    if (slot_lo[c] == slot_lo[c + 1]) continue;
    const uint32_t m_lo = static_cast<uint32_t>(r_base[slot_lo[c]]), m_hi = static_cast<uint32_t>(r_base[slot_lo[c + 1]]);
    const uint32_t per_block = 256 / c;
    // (a class whose streams hold no frame still counts as a launch of the plan: the plan depends on the classes only)
    SB_LAUNCH(streams_decode_kernel, dim3(m_hi > m_lo ? ceil_div(m_hi - m_lo, per_block) : 1), dim3(per_block * c), 0, st,
              d_bytes, descs, perm, base, pcm, f_node, f_slot, s_accepted, cand_pos, recs, m_lo, m_hi, c, where, d_out);
  }
#undef SB_LAUNCH
  HIP_TRY(h, hipGetLastError());
  if (md5) {
    // stream s wrote s_bytes[s] bytes from d_out + where[s] (the compact staging) resp. + its out_offset, the third of
    // the descriptor's six words
    const uint64_t* first = where ? where : reinterpret_cast<const uint64_t*>(descs) + 2;
    HIP_TRY(h, launch_md5_spans(d_out, first, where ? 1u : static_cast<uint32_t>(sizeof(Desc) / 8), s_bytes, nullptr, ns,
                                d_digests, st));
    ++plan[0];
    if (host) {
      HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(h->pin_meta[0]) + result_words * 8, d_digests, n_streams * 16,
                                hipMemcpyDeviceToHost, st));
      ++plan[2];
    }
  }
  if (host) {
    // one transfer of the streams' PCM back to back into pinned staging, then every stream to its slot on the host
    if ((rc = ensure_pinned(h, h->pin_out, &h->pin_out_cap, static_cast<size_t>(pcm_bytes))) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure_copy_pool(h, "decode_streams")) != FLACENC_HIP_OK) return rc;
    if (pcm_bytes) HIP_TRY(h, hipMemcpyAsync(h->pin_out[0], d_out, static_cast<size_t>(pcm_bytes), hipMemcpyDeviceToHost, st));
    ++plan[2];
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
    std::memcpy(totals, r_totals, n_streams * 32);
    if (md5) std::memcpy(digests, static_cast<const char*>(h->pin_meta[0]) + result_words * 8, n_streams * 16);
  }
  call_totals[0] = r_meta[M_FRAMES];
  call_totals[1] = r_meta[M_SAMPLES];
  return FLACENC_HIP_OK;
}

}  // namespace

// ---------------------------------------------------------------- the index, for both calls (stream_index.h)
int streamindex::build(flacenc_hip_handle* h, uint64_t* plan, const Request& rq, Index& ix) {
  const size_t n_streams = rq.n_streams, max_frames = rq.max_frames;
  const uint64_t n_bytes = rq.n_bytes;
  const uint32_t ns = static_cast<uint32_t>(n_streams);
  const bool host = rq.host;
  hipStream_t st = h->stream;
  int rc;

  // ---- the table on its way to the device: the descriptors and the slot order (streams sorted by channel count) ----
  const size_t own_table = (n_streams * sizeof(Desc) + n_streams * 4 + 7) & ~static_cast<size_t>(7);
  const size_t table_bytes = rq.extra_table_bytes ? own_table + rq.extra_table_bytes : n_streams * sizeof(Desc) + n_streams * 4;
  const size_t result_words = M_WORDS + (n_streams + 1) + rq.extra_words;
  const size_t result_bytes = result_words * 8 + rq.pinned_tail;
  if ((rc = ensure_pinned(h, h->pin_meta, &h->pin_meta_cap, table_bytes > result_bytes ? table_bytes : result_bytes)) !=
      FLACENC_HIP_OK)
    return rc;
  Desc* p_desc = static_cast<Desc*>(h->pin_meta[1]);
  uint32_t* p_perm = reinterpret_cast<uint32_t*>(p_desc + n_streams);
  std::memcpy(p_desc, rq.table, n_streams * sizeof(Desc));
  if (rq.extra_table_bytes) std::memcpy(static_cast<char*>(h->pin_meta[1]) + own_table, rq.extra_table, rq.extra_table_bytes);
  uint32_t* slot_lo = ix.slot_lo;  // slots [slot_lo[c], slot_lo[c + 1]) hold the streams of c channels
  for (uint32_t c = 0; c < 10; ++c) slot_lo[c] = 0;
  for (size_t s = 0; s < n_streams; ++s) ++slot_lo[p_desc[s].channels + 1];
  uint32_t classes = 0;
  for (uint32_t c = 1; c <= 8; ++c) {
    classes += slot_lo[c + 1] != 0;
    slot_lo[c + 1] += slot_lo[c];
  }
  {
    uint32_t at[9];
    for (uint32_t c = 1; c <= 8; ++c) at[c] = slot_lo[c];
    for (size_t s = 0; s < n_streams; ++s) p_perm[at[p_desc[s].channels]++] = static_cast<uint32_t>(s);
  }
  ix.classes = classes;
  plan[3] = classes;

  // ---- scratch ----
  const size_t capacity = index_candidate_capacity(max_frames);
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = index_jump_levels(capacity);
  const uint32_t n_blocks = ceil_div(n_bytes, kPosPerBlock);
  const size_t F = max_frames;
  size_t need = 0;
  auto take = [&need](size_t bytes_) {
    const size_t at = need;
    need += a256(bytes_ + 8);
    return at;
  };
  const size_t o_counters = take(256 + M_WORDS * 8 + result_words * 8);  // counters | meta | base | the caller's words
  const size_t o_table = take(table_bytes);
  const size_t o_bcount = take(static_cast<size_t>(n_blocks) * 8), o_boff = take((static_cast<size_t>(n_blocks) + 1) * 8);
  const size_t o_cpos = take(capacity * 8), o_cstream = take(capacity * 4), o_recs = take(capacity * sizeof(FrameRec));
  const size_t o_jump = take(static_cast<size_t>(levels) * capacity * 4);
  const size_t o_sframes = take(n_streams * 8), o_sroot = take(n_streams * 4), o_send = take(n_streams * 8);
  const size_t o_swhy = take(n_streams * 4), o_sacc = take(n_streams * 4), o_sbytes = take(n_streams * 8);
  const size_t o_fnode = take(F * 4), o_fslot = take(F * 4), o_fpcm = take(F * 8), o_fbad = take(F * 8);
  const size_t o_pcm = take((F + 1) * 8), o_bad = take((F + 1) * 8);
  const size_t o_extra = rq.extra_scratch ? take(rq.extra_scratch) : 0;
  if ((rc = ensure(h, h->d_idx, need)) != FLACENC_HIP_OK) return rc;
  char* S = static_cast<char*>(h->d_idx.ptr);
  uint32_t* counters = reinterpret_cast<uint32_t*>(S + o_counters);
  uint64_t* meta = reinterpret_cast<uint64_t*>(S + o_counters + 256);
  uint64_t* base = meta + M_WORDS;
  const Desc* descs = reinterpret_cast<const Desc*>(S + o_table);
  const uint32_t* perm = reinterpret_cast<const uint32_t*>(S + o_table + n_streams * sizeof(Desc));
  uint64_t* block_counts = reinterpret_cast<uint64_t*>(S + o_bcount);
  uint64_t* block_offsets = reinterpret_cast<uint64_t*>(S + o_boff);
  uint64_t* cand_pos = reinterpret_cast<uint64_t*>(S + o_cpos);
  uint32_t* cand_stream = reinterpret_cast<uint32_t*>(S + o_cstream);
  FrameRec* recs = reinterpret_cast<FrameRec*>(S + o_recs);
  uint32_t* jump = reinterpret_cast<uint32_t*>(S + o_jump);
  uint64_t* s_frames = reinterpret_cast<uint64_t*>(S + o_sframes);
  uint32_t* s_root = reinterpret_cast<uint32_t*>(S + o_sroot);
  uint64_t* s_end = reinterpret_cast<uint64_t*>(S + o_send);
  uint32_t* s_why = reinterpret_cast<uint32_t*>(S + o_swhy);
  uint32_t* f_node = reinterpret_cast<uint32_t*>(S + o_fnode);
  uint32_t* f_slot = reinterpret_cast<uint32_t*>(S + o_fslot);
  uint64_t* f_pcm = reinterpret_cast<uint64_t*>(S + o_fpcm);
  uint64_t* f_bad = reinterpret_cast<uint64_t*>(S + o_fbad);
  uint64_t* pcm = reinterpret_cast<uint64_t*>(S + o_pcm);
  uint64_t* bad = reinterpret_cast<uint64_t*>(S + o_bad);
  ix.counters = counters;
  ix.meta = meta;
  ix.base = base;
  ix.extra = base + (n_streams + 1);
  ix.result_words = result_words;
  ix.descs = descs;
  ix.perm = perm;
  ix.extra_table = S + o_table + own_table;
  ix.cap = cap;
  ix.levels = levels;
  ix.cand_pos = cand_pos;
  ix.recs = recs;
  ix.jump = jump;
  ix.s_root = s_root;
  ix.s_why = s_why;
  ix.s_accepted = reinterpret_cast<uint32_t*>(S + o_sacc);
  ix.s_end = s_end;
  ix.s_bytes = reinterpret_cast<uint64_t*>(S + o_sbytes);
  ix.f_node = f_node;
  ix.f_slot = f_slot;
  ix.pcm = pcm;
  ix.bad = bad;
  ix.scratch = S + o_extra;

  // ---- the input ----
  const uint8_t* d_bytes = rq.bytes;
  if (host) {
    if ((rc = ensure(h, h->d_dec_io, static_cast<size_t>(n_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_bytes = static_cast<const uint8_t*>(h->d_dec_io.ptr);
  }
  ix.d_bytes = d_bytes;
#define SB_LAUNCH(...)                 \
  do {                                 \
    hipLaunchKernelGGL(__VA_ARGS__);   \
    ++plan[0];                         \
  } while (0)
  HIP_TRY(h, hipMemsetAsync(counters, 0, 256 + M_WORDS * 8, st));
  HIP_TRY(h, hipMemcpyAsync(S + o_table, p_desc, table_bytes, hipMemcpyHostToDevice, st));
  ++plan[2];
  if (host && n_bytes) {
    const void* src = rq.bytes;
    if (!is_pinned(rq.bytes)) {  // pageable: through pinned staging on the handle's host threads
      if ((rc = ensure_pinned(h, h->pin_in, &h->pin_in_cap, static_cast<size_t>(n_bytes))) != FLACENC_HIP_OK) return rc;
      if ((rc = ensure_copy_pool(h, rq.who)) != FLACENC_HIP_OK) return rc;
      h->copy_pool->copy(h->pin_in[0], rq.bytes, static_cast<size_t>(n_bytes));
      src = h->pin_in[0];
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_dec_io.ptr, src, static_cast<size_t>(n_bytes), hipMemcpyHostToDevice, st));
    ++plan[2];
  }

  // ---- the segmented index ----
  if (n_blocks) {
    SB_LAUNCH(streams_cand_kernel<false>, dim3(n_blocks), dim3(256), 0, st, d_bytes, n_bytes, descs, ns, block_counts,
              nullptr, nullptr, nullptr, cap, counters);
    SB_LAUNCH(streams_scan_kernel, dim3(1), dim3(1024), 0, st, block_counts, nullptr, nullptr,
              static_cast<uint64_t>(n_blocks), nullptr, block_offsets, nullptr);
    SB_LAUNCH(streams_cand_kernel<true>, dim3(n_blocks), dim3(256), 0, st, d_bytes, n_bytes, descs, ns, nullptr,
              block_offsets, cand_pos, cand_stream, cap, counters);
    SB_LAUNCH(streams_skim_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st, d_bytes, descs, cand_pos, cand_stream,
              counters, cap, recs);
    HIP_TRY(h, launch_frame_crc16(d_bytes, cand_pos, cap, counters + C_CANDS, recs, st));
    ++plan[0];
    SB_LAUNCH(streams_link_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st, descs, cand_pos, cand_stream, recs,
              counters, cap, jump);
    HIP_TRY(h, launch_jump_levels(jump, counters + C_CANDS, capacity, st));
    plan[0] += levels - 1;
  }
  SB_LAUNCH(streams_chain_kernel, dim3(ceil_div(ns, 256)), dim3(256), 0, st, descs, ns, cand_pos, recs, jump, levels,
            counters, cap, s_frames, s_root, s_end, s_why);
  SB_LAUNCH(streams_scan_kernel, dim3(1), dim3(1024), 0, st, s_frames, nullptr, perm, static_cast<uint64_t>(ns), nullptr,
            base, nullptr);
  SB_LAUNCH(streams_verdict_kernel, dim3(1), dim3(1), 0, st, base, ns, static_cast<uint64_t>(max_frames), cap, counters,
            meta);
  // ---- every chain frame, and the scans over the frame sequence ----
  if (F)
    SB_LAUNCH(streams_enumerate_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, st, descs, perm, ns, base, s_root, recs,
              jump, levels, counters, cap, f_node, f_slot, f_pcm, f_bad);
  SB_LAUNCH(streams_scan_kernel, dim3(1), dim3(1024), 0, st, f_pcm, f_bad, nullptr, static_cast<uint64_t>(F),
            counters + C_FRAMES, pcm, bad);
#undef SB_LAUNCH
  return FLACENC_HIP_OK;
}

hipError_t streamindex::launch_scan2(const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out_a, uint64_t* out_b,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(streams_scan_kernel, dim3(1), dim3(1024), 0, stream, a, b, nullptr, n, nullptr, out_a, out_b);
  return hipGetLastError();
}

// streams_scan_kernel for the batch encoder (encode_streams.cpp): out[i] = the sum of in[j] over j < i, out[n] the total
hipError_t launch_streams_scan(const uint64_t* in, uint64_t n, uint64_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(streams_scan_kernel, dim3(1), dim3(1024), 0, stream, in, nullptr, nullptr, n, nullptr, out, nullptr);
  return hipGetLastError();
}

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
