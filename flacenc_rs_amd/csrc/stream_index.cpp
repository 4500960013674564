// stream_index.cpp -- the decoder's frame index (stream_index.h): launch_index_frames for one stream and
// streamindex::build for a batch of streams, on one pipeline.
//
// A byte position is a candidate when it lies inside a span and a valid header for that span's parameters starts
// there; candidates are compacted in ascending order (count per workgroup, scan, write), each is skimmed and CRC-checked
// up to its span's end and linked to the verified candidate that starts where it ends ("ends at the span's end" is the
// end sentinel); jump levels follow by pointer jumping.  Which span holds a byte, and a span's end and parameters, is
// all these kernels ask: a span policy answers it, OneSpan for the single stream [0, n_bytes) and TableSpans for a
// descriptor table.  (The skim of the single stream is the one kernel that is not shared: it stays skim_kernel's index
// mode in flac_decode.cpp, see launch_skim.)  What is read off the links differs and stays apart:
//   chain_kernel, enumerate_kernel                   one stream: the chain from byte 0, a verified prefix with the flag
//                                                    on its count, clamped at max_frames
//   streams_chain_kernel .. streams_enumerate_kernel a batch: every stream has its own chain root, the verified
//                                                    candidate at its first byte; one lane per stream measures its
//                                                    chain, a scan over streams (in `slot` order: the table sorted by
//                                                    channel count) gives frame bases, the verdict ends the whole call
//                                                    on too many frames or candidates, every frame of every stream is
//                                                    enumerated by its own lane, and two scans run over the frame
//                                                    sequence (PCM bytes, frames with a status)
#include "stream_index.h"

#include "flac_decode.h"
#include "flac_decode_device.h"

namespace flacenc_hip {
namespace {

using namespace streamindex;  // the counters' and meta words' names

using flacdec::FrameRec;
using Desc = flacenc_hip_stream_desc;

__constant__ flacdec::CrcTables kCrc = flacdec::make_crc_tables();

constexpr uint64_t kIndexError = 0x8000000000000000ull;  // FLACENC_HIP_INDEX_ERROR

// ---------------------------------------------------------------- span policies
struct Span {
  uint64_t end;  // the first byte behind the span
  uint32_t channels, bps, max_bps;  // max_bps: the handle's depth limit, the same for every span of a call
};

// a descriptor table; cand_stream[i] remembers the stream of candidate i
struct TableSpans {
  const Desc* descs;
  uint32_t n_streams;
  uint32_t* cand_stream;
  uint32_t max_bps;
  __device__ uint32_t find(uint64_t p) const { return streambatch::stream_of_byte(descs, n_streams, p); }
  __device__ Span span(uint32_t s) const {
    return {descs[s].offset + descs[s].n_bytes, descs[s].channels, descs[s].bits_per_sample, max_bps};
  }
  __device__ void keep(uint32_t i, uint32_t s) const { cand_stream[i] = s; }
  __device__ Span of_candidate(uint32_t i) const { return span(cand_stream[i]); }
};

// one stream: [0, n_bytes)
struct OneSpan {
  uint64_t n_bytes;
  uint32_t channels, bps, max_bps;
  __device__ uint32_t find(uint64_t p) const { return p < n_bytes ? 0u : streambatch::NONE; }
  __device__ Span span(uint32_t) const { return {n_bytes, channels, bps, max_bps}; }
  __device__ void keep(uint32_t, uint32_t) const {}
  __device__ Span of_candidate(uint32_t) const { return span(0); }
};

// ---------------------------------------------------------------- candidates
// does a valid header of the span that holds byte p start there?  The policy is consulted only behind the sync test.
template <class Spans>
__device__ bool is_candidate(const uint8_t* bytes, uint64_t n_bytes, const Spans& spans, uint64_t p) {
  if (p + 1 >= n_bytes || bytes[p] != 0xFFu || (bytes[p + 1] & 0xFEu) != 0xF8u) return false;
  const uint32_t s = spans.find(p);
  if (s == streambatch::NONE) return false;
  const Span x = spans.span(s);
  const uint64_t left = x.end - p;  // what the parse may read ends with the span
  flacdec::Header h;
  return flacdec::parse_header(bytes + p, left > 64 ? 64u : static_cast<uint32_t>(left), x.channels, x.bps, 65536u,
                               x.max_bps, kCrc, h) == 0;
}

// WRITE false: block_counts[block] = its candidates.  WRITE true: block_offsets (their exclusive scan) in, the
// candidates' positions (and, with the policy, their spans) out in ascending order, and the total in counters[C_CANDS]
template <class Spans, bool WRITE>
__global__ void __launch_bounds__(256) streams_cand_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                           Spans spans, uint64_t* __restrict__ block_counts,
                                                           const uint64_t* __restrict__ block_offsets,
                                                           uint64_t* __restrict__ cand_pos, uint32_t capacity,
                                                           uint32_t* __restrict__ counters) {
  __shared__ uint32_t sh[256];
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock + threadIdx.x * kPosPerThread;
  uint32_t mask = 0;
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if (is_candidate(bytes, n_bytes, spans, base + k)) mask |= 1u << k;
  uint32_t total;
  const uint32_t before = block_scan(__popc(mask), sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
    return;
  }
  const uint64_t first = block_offsets[blockIdx.x] + before;
  // positions ascend, so whatever lies past `capacity` is dropped
  uint32_t at = first < capacity ? static_cast<uint32_t>(first) : capacity;
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if (((mask >> k) & 1u) && at < capacity) {
      cand_pos[at] = base + k;
      spans.keep(at, spans.find(base + k));
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

// ---------------------------------------------------------------- skim and link, per candidate with its span
// candidate i may run to its stream's end; its parsed length is recorded.  NUMBERS: its coded number and blocking bit
// (bit 0 of the header's second byte) too, numbers[i] = number << 1 | bit
template <bool NUMBERS>
__global__ void __launch_bounds__(256) streams_skim_kernel(const uint8_t* __restrict__ bytes, TableSpans spans,
                                                           const uint64_t* __restrict__ cand_pos,
                                                           const uint32_t* __restrict__ counters, uint32_t capacity,
                                                           FrameRec* __restrict__ recs, uint64_t* __restrict__ numbers) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Span x = spans.of_candidate(i);
  const uint64_t off = cand_pos[i], left = x.end - off;  // a candidate lies inside its span
  FrameRec rec;
  uint64_t number = 0;
  flacdec::skim_frame(bytes + off, left > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(left), x.channels, x.bps,
                      65536u, x.max_bps, false, kCrc, rec, NUMBERS ? &number : nullptr);
  recs[i] = rec;
  if (NUMBERS) numbers[i] = number << 1 | (bytes[off + 1] & 1u);
}

// The skim of a table takes each candidate's parameters from its stream.  The single stream keeps skim_kernel's index
// mode (flac_decode.cpp), whose parameters are the launch's: that kernel is measurably faster there (about 1.5 % of a
// skim that is 70 % of flacenc_hip_index_frames) than this one compiled for one span.
void launch_skim(const uint8_t* bytes, uint64_t, const TableSpans& spans, const uint64_t* cand_pos,
                 const uint32_t* counters, uint32_t cap, FrameRec* recs, uint64_t* numbers, hipStream_t st) {
  if (numbers)
    hipLaunchKernelGGL(streams_skim_kernel<true>, dim3(ceil_div(cap, 256)), dim3(256), 0, st, bytes, spans, cand_pos,
                       counters, cap, recs, numbers);
  else
    hipLaunchKernelGGL(streams_skim_kernel<false>, dim3(ceil_div(cap, 256)), dim3(256), 0, st, bytes, spans, cand_pos,
                       counters, cap, recs, numbers);
}
void launch_skim(const uint8_t* bytes, uint64_t n_bytes, const OneSpan& spans, const uint64_t* cand_pos,
                 const uint32_t* counters, uint32_t cap, FrameRec* recs, uint64_t*, hipStream_t st) {
  (void)launch_frame_skim(bytes, n_bytes, cand_pos, cap, counters + C_CANDS, spans.channels, spans.bps, spans.max_bps,
                          recs, st);
}

// jump[0][i]: the verified candidate that starts where candidate i ends, kEnd at its span's end, kDead otherwise -- so a
// chain only ever walks over verified frames, also when candidates were dropped at `capacity`.  A frame ends inside its
// span and spans do not overlap, so the candidate found there belongs to the same span.
template <class Spans>
__global__ void __launch_bounds__(256) streams_link_kernel(Spans spans, const uint64_t* __restrict__ cand_pos,
                                                           const FrameRec* __restrict__ recs,
                                                           const uint32_t* __restrict__ counters, uint32_t capacity,
                                                           uint32_t* __restrict__ jump) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = kDead;
  if (recs[i].status == 0) {
    const uint64_t e = cand_pos[i] + recs[i].len;
    nx = e == spans.of_candidate(i).end ? kEnd : verified_at(cand_pos, recs, i + 1, n, e);
  }
  jump[i] = nx;
}

// The resynchronising forms (Request::resync).  The verified candidates are ranked first: v_flag[i] = 1 for a verified
// candidate, v_rank its exclusive scan (streams_scan_kernel), v_list[v_rank[i]] = i -- so the first verified candidate at
// or behind candidate j is v_list[v_rank[j]], whatever lies unverified between them.
__global__ void __launch_bounds__(256) resync_flag_kernel(const FrameRec* __restrict__ recs,
                                                          const uint32_t* __restrict__ counters, uint32_t capacity,
                                                          uint64_t* __restrict__ v_flag) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v_flag[i] = recs[i].status == 0 ? 1u : 0u;
}

__global__ void __launch_bounds__(256) resync_list_kernel(const FrameRec* __restrict__ recs,
                                                          const uint64_t* __restrict__ v_rank,
                                                          const uint32_t* __restrict__ counters, uint32_t capacity,
                                                          uint32_t* __restrict__ v_list) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && recs[i].status == 0) v_list[v_rank[i]] = i;
}

// the first verified candidate of [lo, n) at or behind byte x and in front of byte `end`; kDead if there is none
__device__ inline uint32_t resync_at(const uint64_t* cand_pos, const uint64_t* v_rank, const uint32_t* v_list,
                                     uint32_t lo, uint32_t n, uint64_t x, uint64_t end) {
  const uint32_t j = lower_bound(cand_pos, lo, n, x);
  const uint64_t r = v_rank[j];  // v_rank has n + 1 words
  if (r >= v_rank[n]) return kDead;
  const uint32_t k = v_list[r];
  return cand_pos[k] < end ? k : kDead;
}

// jump[0][i] of the resynchronising chain: the first verified candidate at or behind the end of verified candidate i
// inside its span, kEnd when the span holds none; kDead for an unverified candidate.  The candidate found starts at or
// behind a byte of the span and in front of the span's end, so it belongs to the same span.
__global__ void __launch_bounds__(256) streams_resync_link_kernel(TableSpans spans, const uint64_t* __restrict__ cand_pos,
                                                                  const FrameRec* __restrict__ recs,
                                                                  const uint64_t* __restrict__ v_rank,
                                                                  const uint32_t* __restrict__ v_list,
                                                                  const uint32_t* __restrict__ counters,
                                                                  uint32_t capacity, uint32_t* __restrict__ jump) {
  const uint32_t n = min(counters[C_CANDS], capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = kDead;
  if (recs[i].status == 0) {
    nx = resync_at(cand_pos, v_rank, v_list, i + 1, n, cand_pos[i] + recs[i].len, spans.of_candidate(i).end);
    if (nx == kDead) nx = kEnd;
  }
  jump[i] = nx;
}

__global__ void __launch_bounds__(256) jump_kernel(const uint32_t* __restrict__ prev, uint32_t* __restrict__ next,
                                                   const uint32_t* __restrict__ n_dev, uint32_t capacity) {
  const uint32_t n = min(*n_dev, capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = prev[i];
  next[i] = a >= kEnd ? a : prev[a];
}

uint32_t jump_levels(size_t capacity) {
  uint32_t l = 1;
  while ((static_cast<size_t>(1) << l) <= capacity) ++l;
  return l;
}

// what the resynchronising index adds to the pipeline: the candidates' numbers and the ranking of the verified ones
struct Resync {
  uint64_t *numbers, *v_flag, *v_rank;  // [capacity], [capacity], [capacity + 1]
  uint32_t* v_list;                     // [capacity]
  void link(const TableSpans& spans, const uint64_t* cand_pos, const FrameRec* recs, const uint32_t* counters,
            uint32_t cap, uint32_t* jump, hipStream_t st) const {
    hipLaunchKernelGGL(streams_resync_link_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st, spans, cand_pos, recs,
                       v_rank, v_list, counters, cap, jump);
  }
  void link(const OneSpan&, const uint64_t*, const FrameRec*, const uint32_t*, uint32_t, uint32_t*, hipStream_t) const {}
};

// The pipeline both indexes queue on `stream`: n_blocks > 0 workgroups of candidates into cand_pos[capacity], their skim
// records and the jump levels.  Every launch is added to plan[0] when a plan is given.
template <class Spans>
hipError_t launch_links(const uint8_t* bytes, uint64_t n_bytes, const Spans& spans, uint32_t n_blocks,
                        uint64_t* block_counts, uint64_t* block_offsets, uint64_t* cand_pos, FrameRec* recs,
                        uint32_t* jump, uint32_t* counters, size_t capacity, uint64_t* plan, hipStream_t st,
                        const Resync* resync = nullptr) {
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = jump_levels(capacity);
  uint64_t uncounted[1];
  uint64_t* count = plan ? plan : uncounted;
  COUNTED_LAUNCH(count, (streams_cand_kernel<Spans, false>), dim3(n_blocks), dim3(256), 0, st, bytes, n_bytes, spans,
                 block_counts, nullptr, nullptr, cap, counters);
  COUNTED_LAUNCH(count, streams_scan_kernel, dim3(1), dim3(1024), 0, st, block_counts, nullptr, nullptr,
                 static_cast<uint64_t>(n_blocks), nullptr, block_offsets, nullptr);
  COUNTED_LAUNCH(count, (streams_cand_kernel<Spans, true>), dim3(n_blocks), dim3(256), 0, st, bytes, n_bytes, spans,
                 nullptr, block_offsets, cand_pos, cap, counters);
  launch_skim(bytes, n_bytes, spans, cand_pos, counters, cap, recs, resync ? resync->numbers : nullptr, st);
  ++count[0];
  hipError_t e = launch_frame_crc16(bytes, cand_pos, cap, counters + C_CANDS, recs, st);
  if (e != hipSuccess) return e;
  ++count[0];
  if (resync) {
    COUNTED_LAUNCH(count, resync_flag_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st, recs, counters, cap,
                   resync->v_flag);
    COUNTED_LAUNCH(count, streams_scan_kernel, dim3(1), dim3(1024), 0, st, resync->v_flag, nullptr, nullptr,
                   static_cast<uint64_t>(cap), counters + C_CANDS, resync->v_rank, nullptr);
    COUNTED_LAUNCH(count, resync_list_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st, recs, resync->v_rank, counters,
                   cap, resync->v_list);
    resync->link(spans, cand_pos, recs, counters, cap, jump, st);
    ++count[0];
  } else {
    COUNTED_LAUNCH(count, streams_link_kernel<Spans>, dim3(ceil_div(cap, 256)), dim3(256), 0, st, spans, cand_pos, recs,
                   counters, cap, jump);
  }
  for (uint32_t k = 1; k < levels; ++k)
    COUNTED_LAUNCH(count, jump_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, st,
                   jump + static_cast<size_t>(k - 1) * cap, jump + static_cast<size_t>(k) * cap, counters + C_CANDS, cap);
  return hipGetLastError();
}

// ---------------------------------------------------------------- one stream: the chain from byte 0
// one thread: the length of the chain from the candidate at byte 0
__global__ void chain_kernel(const uint64_t* __restrict__ cand_pos, const FrameRec* __restrict__ recs,
                             const uint32_t* __restrict__ jump, uint32_t levels, uint32_t* __restrict__ counters,
                             uint32_t capacity, uint64_t n_bytes, uint64_t max_frames,
                             uint64_t* __restrict__ n_frames) {
  const uint32_t total = counters[C_CANDS], n = min(total, capacity);
  // candidates past `capacity` (the highest positions) were dropped: what the chain reaches is still a verified
  // prefix, but it may stop early, so the caller is told to come back with a larger max_frames
  uint64_t err = total > capacity ? kIndexError : 0;
  uint64_t count = 0;
  if (n_bytes == 0) {
    // an empty buffer holds no frame and no error
  } else if (n == 0 || cand_pos[0] != 0 || recs[0].status != 0) {
    err = kIndexError;  // no verified frame at byte 0
  } else {
    const ChainEnd c = walk_chain(jump, levels, capacity, 0);
    count = c.count;
    if (jump[c.last] != kEnd) err = kIndexError;
    if (count > max_frames) {
      err = kIndexError;
      count = max_frames;
    }
  }
  counters[1] = static_cast<uint32_t>(count);
  *n_frames = count | err;
}

__global__ void __launch_bounds__(256) enumerate_kernel(const uint64_t* __restrict__ cand_pos,
                                                        const FrameRec* __restrict__ recs,
                                                        const uint32_t* __restrict__ jump, uint32_t levels,
                                                        const uint32_t* __restrict__ counters, uint32_t capacity,
                                                        uint64_t* __restrict__ offsets, uint32_t* __restrict__ lengths) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= counters[1]) return;
  const uint32_t node = chain_node(jump, levels, capacity, 0, m);
  offsets[m] = cand_pos[node];
  lengths[m] = recs[node].len;
}

// ---------------------------------------------------------------- a batch: one lane per stream
// RESYNC: the root is the first verified candidate of the span (v_rank, v_list: see resync_flag_kernel) and the chain
// never ends with a reason.
template <bool RESYNC>
__global__ void __launch_bounds__(256) streams_chain_kernel(const Desc* __restrict__ descs, uint32_t n_streams,
                                                            const uint64_t* __restrict__ cand_pos,
                                                            const FrameRec* __restrict__ recs,
                                                            const uint32_t* __restrict__ jump, uint32_t levels,
                                                            const uint32_t* __restrict__ counters, uint32_t capacity,
                                                            uint64_t* __restrict__ s_frames, uint32_t* __restrict__ s_root,
                                                            uint64_t* __restrict__ s_end, uint32_t* __restrict__ s_why,
                                                            const uint64_t* __restrict__ v_rank,
                                                            const uint32_t* __restrict__ v_list) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  const Desc& d = descs[s];
  const uint32_t n = min(counters[C_CANDS], capacity);
  uint64_t count = 0, end = d.offset;
  uint32_t root = kDead, why = 0;
  if (d.n_bytes != 0) {
    // the verified candidate at the stream's first byte
    root = RESYNC ? resync_at(cand_pos, v_rank, v_list, 0, n, d.offset, d.offset + d.n_bytes)
                  : verified_at(cand_pos, recs, 0, n, d.offset);
    if (root == kDead) {
      why = RESYNC ? 0u : static_cast<uint32_t>(FLACENC_HIP_DECODE_CHAIN);
    } else {
      const ChainEnd c = walk_chain(jump, levels, capacity, root);
      count = c.count;
      end = cand_pos[c.last] + recs[c.last].len;
      if (!RESYNC && jump[c.last] != kEnd) why = FLACENC_HIP_DECODE_CHAIN;
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
  const uint32_t node = chain_node(jump, levels, capacity, s_root[s], m - static_cast<uint32_t>(base[i]));
  const Desc& d = descs[s];
  const uint32_t bs = recs[node].block_size;
  f_node[m] = node;
  f_slot[m] = i;
  f_pcm[m] = static_cast<uint64_t>(bs) * d.channels * d.bytes_per_sample;
  f_bad[m] = bs > d.max_block_size ? 1u : 0u;
}

}  // namespace

// ---------------------------------------------------------------- flacenc_hip_index_frames
size_t index_candidate_capacity(size_t max_frames) { return max_frames + max_frames / 4 + 4096; }

// block counts | their scan | counters | cand_pos | recs | jump levels
size_t index_scratch_bytes(uint64_t n_bytes, size_t capacity) {
  const size_t n_blocks = (n_bytes + kPosPerBlock - 1) / kPosPerBlock;
  return a256(n_blocks * 8) + a256((n_blocks + 1) * 8) + 256 + a256(capacity * 8) + a256(capacity * sizeof(FrameRec)) +
         static_cast<size_t>(jump_levels(capacity)) * capacity * 4;
}

hipError_t launch_index_frames(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bps,
                               uint32_t max_bps, size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames,
                               void* scratch, size_t capacity, hipStream_t stream) {
  const uint32_t n_blocks = ceil_div(n_bytes, kPosPerBlock);
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = jump_levels(capacity);
  char* s = static_cast<char*>(scratch);
  uint64_t* block_counts = reinterpret_cast<uint64_t*>(s);
  s += a256(static_cast<size_t>(n_blocks) * 8);
  uint64_t* block_offsets = reinterpret_cast<uint64_t*>(s);
  s += a256((static_cast<size_t>(n_blocks) + 1) * 8);
  uint32_t* counters = reinterpret_cast<uint32_t*>(s);
  s += 256;
  uint64_t* cand_pos = reinterpret_cast<uint64_t*>(s);
  s += a256(capacity * 8);
  FrameRec* recs = reinterpret_cast<FrameRec*>(s);
  s += a256(capacity * sizeof(FrameRec));
  uint32_t* jump = reinterpret_cast<uint32_t*>(s);
  hipError_t e = hipMemsetAsync(counters, 0, 256, stream);
  if (e != hipSuccess) return e;
  if (n_blocks) {
    e = launch_links(bytes, n_bytes, OneSpan{n_bytes, channels, bps, max_bps}, n_blocks, block_counts, block_offsets, cand_pos,
                     recs, jump, counters, capacity, nullptr, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(1), 0, stream, cand_pos, recs, jump, levels, counters, cap, n_bytes,
                     static_cast<uint64_t>(max_frames), n_frames);
  if (max_frames)
    hipLaunchKernelGGL(enumerate_kernel, dim3(ceil_div(max_frames < cap ? max_frames : cap, 256)), dim3(256), 0, stream,
                       cand_pos, recs, jump, levels, counters, cap, offsets, lengths);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the index of a batch, for both calls
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
  ix.classes = sort_by_channels(n_streams, [p_desc](size_t s) { return p_desc[s].channels; }, ix.slot_lo, p_perm);
  plan[3] = ix.classes;

  // ---- scratch ----
  const size_t capacity = index_candidate_capacity(max_frames);
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = jump_levels(capacity);
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
  // (behind everything the other calls lay out, so that their layout is what it was)
  const size_t o_num = rq.resync ? take(capacity * 8) : 0, o_vflag = rq.resync ? take(capacity * 8) : 0;
  const size_t o_vrank = rq.resync ? take((capacity + 1) * 8) : 0, o_vlist = rq.resync ? take(capacity * 4) : 0;
  if ((rc = ensure(h, h->d_idx, need)) != FLACENC_HIP_OK) return rc;
  char* S = static_cast<char*>(h->d_idx.ptr);
  uint32_t* counters = reinterpret_cast<uint32_t*>(S + o_counters);
  uint64_t* meta = reinterpret_cast<uint64_t*>(S + o_counters + 256);
  uint64_t* base = meta + M_WORDS;
  const Desc* descs = reinterpret_cast<const Desc*>(S + o_table);
  const uint32_t* perm = reinterpret_cast<const uint32_t*>(S + o_table + n_streams * sizeof(Desc));
  uint64_t* cand_pos = reinterpret_cast<uint64_t*>(S + o_cpos);
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
  const Resync resync{reinterpret_cast<uint64_t*>(S + o_num), reinterpret_cast<uint64_t*>(S + o_vflag),
                      reinterpret_cast<uint64_t*>(S + o_vrank), reinterpret_cast<uint32_t*>(S + o_vlist)};
  ix.cand_number = rq.resync ? resync.numbers : nullptr;

  // ---- the input ----
  const uint8_t* d_bytes = rq.bytes;
  if (host) {
    if ((rc = ensure(h, h->d_dec_io, static_cast<size_t>(n_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_bytes = static_cast<const uint8_t*>(h->d_dec_io.ptr);
  }
  ix.d_bytes = d_bytes;
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
  if (n_blocks)
    HIP_TRY(h, launch_links(d_bytes, n_bytes, TableSpans{descs, ns, reinterpret_cast<uint32_t*>(S + o_cstream), h->max_bps}, n_blocks,
                            reinterpret_cast<uint64_t*>(S + o_bcount), reinterpret_cast<uint64_t*>(S + o_boff), cand_pos,
                            recs, jump, counters, capacity, plan, st, rq.resync ? &resync : nullptr));
  if (rq.resync) {
    // (no candidate pass ran on an input of 0 bytes: the ranking the root choice reads is then the empty one)
    if (!n_blocks) HIP_TRY(h, hipMemsetAsync(resync.v_rank, 0, 8, st));
    COUNTED_LAUNCH(plan, streams_chain_kernel<true>, dim3(ceil_div(ns, 256)), dim3(256), 0, st, descs, ns, cand_pos, recs,
                   jump, levels, counters, cap, s_frames, s_root, s_end, s_why, resync.v_rank, resync.v_list);
  } else {
    COUNTED_LAUNCH(plan, streams_chain_kernel<false>, dim3(ceil_div(ns, 256)), dim3(256), 0, st, descs, ns, cand_pos, recs,
                   jump, levels, counters, cap, s_frames, s_root, s_end, s_why, nullptr, nullptr);
  }
  COUNTED_LAUNCH(plan, streams_scan_kernel, dim3(1), dim3(1024), 0, st, s_frames, nullptr, perm,
                 static_cast<uint64_t>(ns), nullptr, base, nullptr);
  COUNTED_LAUNCH(plan, streams_verdict_kernel, dim3(1), dim3(1), 0, st, base, ns, static_cast<uint64_t>(max_frames), cap,
                 counters, meta);
  // ---- every chain frame, and the scans over the frame sequence ----
  if (F)
    COUNTED_LAUNCH(plan, streams_enumerate_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, st, descs, perm, ns, base, s_root,
                   recs, jump, levels, counters, cap, f_node, f_slot, f_pcm, f_bad);
  COUNTED_LAUNCH(plan, streams_scan_kernel, dim3(1), dim3(1024), 0, st, f_pcm, f_bad, nullptr, static_cast<uint64_t>(F),
                 counters + C_FRAMES, pcm, bad);
  return FLACENC_HIP_OK;
}

hipError_t streamindex::launch_scan2(const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out_a, uint64_t* out_b,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(streams_scan_kernel, dim3(1), dim3(1024), 0, stream, a, b, nullptr, n, nullptr, out_a, out_b);
  return hipGetLastError();
}

hipError_t streamindex::launch_scan2_dev(const uint64_t* a, const uint64_t* b, uint64_t n, const uint32_t* n_dev,
                                         uint64_t* out_a, uint64_t* out_b, hipStream_t stream) {
  hipLaunchKernelGGL(streams_scan_kernel, dim3(1), dim3(1024), 0, stream, a, b, nullptr, n, n_dev, out_a, out_b);
  return hipGetLastError();
}

int streamindex::download_pcm(flacenc_hip_handle* h, uint64_t* plan, const char* who, const uint8_t* d_out,
                              uint64_t pcm_bytes) {
  int rc;
  if ((rc = ensure_pinned(h, h->pin_out, &h->pin_out_cap, static_cast<size_t>(pcm_bytes))) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure_copy_pool(h, who)) != FLACENC_HIP_OK) return rc;
  if (pcm_bytes)
    HIP_TRY(h, hipMemcpyAsync(h->pin_out[0], d_out, static_cast<size_t>(pcm_bytes), hipMemcpyDeviceToHost, h->stream));
  ++plan[2];
  return FLACENC_HIP_OK;
}

}  // namespace flacenc_hip
