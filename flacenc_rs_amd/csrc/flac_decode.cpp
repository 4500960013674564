// flac_decode.cpp -- decode, verify and index FLAC frames on the GPU (flacenc_hip_decode_frames and friends).
//
// Frames are independent, so the work spreads over frames; inside a subframe the LPC recurrence is serial and not
// linear, so a subframe is one lane's work.  Three kernels per launch:
//   skim_kernel      one lane per frame: the header, then every subframe's codes without reconstruction (unary codes
//                    by clz on a 64-bit window), recording where each subframe starts (flacdec::skim_frame)
//   crc16_kernel     one wave per frame: the frame's CRC-16 in 64 strided pieces, combined by x^(8 len) mod P
//   subframe_kernel  one lane per subframe, a frame's channels on adjacent lanes: SubDecoder<MAXP> with the last MAXP
//                    samples in registers (MAXP = the wave's largest order bucket); stereo is undone with a lane
//                    exchange on every sample; 16 samples per lane are staged in LDS so that every store (decode) or
//                    load of the expected samples (verify) moves 64 bytes of one row
// Indexing finds candidate headers at every byte, compacts them in order, skims and CRC-checks each, links each to
// the candidate that starts where it ends and resolves the chain from byte 0 by pointer jumping.
#include "flac_decode.h"

#include "flac_decode_core.h"

namespace flacenc_hip {
namespace {

using flacdec::FrameRec;

__constant__ flacdec::CrcTables kCrc = flacdec::make_crc_tables();

constexpr uint32_t kEnd = 0xFFFFFFFEu, kDead = 0xFFFFFFFFu;  // chain sentinels
constexpr uint64_t kIndexError = 0x8000000000000000ull;      // FLACENC_HIP_INDEX_ERROR
constexpr int kStage = 20;                                   // LDS words per lane (16 staged samples, padded)

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

// ---------------------------------------------------------------- skim: one lane per frame
// index mode (lengths == NULL): frame i starts at offsets[i], may run to n_bytes, and its parsed length is recorded
__global__ void __launch_bounds__(256) skim_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                   const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lengths, uint32_t n,
                                                   const uint32_t* __restrict__ n_dev, uint32_t channels, uint32_t bps,
                                                   uint32_t max_block_size, FrameRec* __restrict__ recs,
                                                   uint64_t* __restrict__ nums) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) n = min(n, *n_dev);
  if (f >= n) return;
  const uint64_t off = offsets[f];
  FrameRec rec;
  uint64_t num = 0;
  uint32_t len;
  if (lengths) {
    len = lengths[f];
  } else {
    const uint64_t left = off < n_bytes ? n_bytes - off : 0;
    len = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(left);
  }
  if (off > n_bytes || len > n_bytes - off) {
    for (uint32_t c = 0; c < flacdec::MAX_CHANNELS; ++c) rec.sub_bit[c] = 0;
    rec.status = flacdec::LENGTH;
    rec.block_size = rec.info = rec.len = 0;
  } else {
    flacdec::skim_frame(bytes + off, len, channels, bps, max_block_size, lengths != nullptr, kCrc, rec, &num);
  }
  recs[f] = rec;
  if (nums) nums[f] = num;
}

// ---------------------------------------------------------------- CRC-16: one wave per frame
// The frame's first len - 2 bytes are read as if preceded by `pad` zero bytes (which leave a CRC with init 0 as it
// is) so that they fill R rounds of 256 bytes; lane i takes bytes 4i .. 4i + 3 of every round.  Its accumulator
// advances by 256 bytes per round (klo / khi tables) and finally by the 252 - 4i bytes that follow its last word
// (xp); the XOR of the 64 accumulators is the frame's CRC.
__global__ void __launch_bounds__(256) crc16_kernel(const uint8_t* __restrict__ bytes,
                                                    const uint64_t* __restrict__ offsets, uint32_t n,
                                                    const uint32_t* __restrict__ n_dev, FrameRec* __restrict__ recs) {
  __shared__ uint16_t t16[256], klo[256], khi[256];
  t16[threadIdx.x] = kCrc.t16[threadIdx.x];
  klo[threadIdx.x] = kCrc.klo[threadIdx.x];
  khi[threadIdx.x] = kCrc.khi[threadIdx.x];
  __syncthreads();
  if (n_dev) n = min(n, *n_dev);
  const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (f >= n) return;
  const uint32_t st = recs[f].status, flen = recs[f].len;
  if (st != 0) return;
  const uint8_t* p = bytes + offsets[f];
  const uint32_t L = flen - 2;
  const uint32_t rounds = (L + 255) / 256;
  const int64_t pad = static_cast<int64_t>(rounds) * 256 - L;
  uint32_t acc = 0;
  for (uint32_t r = 0; r < rounds; ++r) {
    const int64_t q = static_cast<int64_t>(r) * 256 + 4 * lane - pad;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t b = q + k >= 0 ? p[q + k] : 0u;
      w = ((w << 8) & 0xFFFFu) ^ t16[((w >> 8) ^ b) & 0xFFu];
    }
    acc = klo[acc & 0xFFu] ^ khi[acc >> 8] ^ w;
  }
  acc = flacdec::crc16_mulmod(acc, kCrc.xp[lane]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc ^= __shfl_xor(acc, m);
  if (lane == 0 && acc != ((static_cast<uint32_t>(p[L]) << 8) | p[L + 1])) recs[f].status = flacdec::FRAME_CRC;
}

// ---------------------------------------------------------------- reconstruction: one lane per subframe
template <int MAXP, bool VERIFY>
__device__ bool run_subframe(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t sbps,
                             uint32_t ch_tag, uint32_t c, int32_t* row, const int32_t* erow, int32_t* stage) {
  flacdec::SubDecoder<MAXP> d;
  if (bs) d.init(fp, flen, start, bs, sbps);
  const bool stereo = ch_tag >= 8;
  const int32_t* mem = VERIFY ? erow : row;
  const bool vec = (reinterpret_cast<uintptr_t>(mem) & 15u) == 0;
  bool bad = false;
  for (uint32_t t0 = 0; t0 < bs; t0 += 16) {
    const uint32_t m = min(16u, bs - t0);
    for (uint32_t i = 0; i < m; ++i) {
      int32_t v = d.next();
      if (stereo) {
        const int32_t o = __shfl_xor(v, 1);
        int32_t a = c == 0 ? v : o, b = c == 0 ? o : v;
        flacdec::undo_stereo(ch_tag, a, b);
        v = c == 0 ? a : b;
      }
      stage[i] = v;
    }
    if (vec && m == 16) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int4 s = *reinterpret_cast<const int4*>(stage + 4 * k);
        if (VERIFY) {
          const int4 e = *reinterpret_cast<const int4*>(erow + t0 + 4 * k);
          bad |= (s.x != e.x) | (s.y != e.y) | (s.z != e.z) | (s.w != e.w);
        } else {
          *reinterpret_cast<int4*>(row + t0 + 4 * k) = s;
        }
      }
    } else {
      for (uint32_t i = 0; i < m; ++i) {
        if (VERIFY) bad |= stage[i] != erow[t0 + i];
        else row[t0 + i] = stage[i];
      }
    }
  }
  return bad;
}

template <bool VERIFY>
__global__ void __launch_bounds__(256) subframe_kernel(const uint8_t* __restrict__ bytes,
                                                       const uint64_t* __restrict__ offsets,
                                                       const FrameRec* __restrict__ recs,
                                                       const uint64_t* __restrict__ nums, uint32_t n_frames,
                                                       uint32_t channels, uint32_t bps, uint32_t max_block_size,
                                                       int32_t* __restrict__ out, const int32_t* __restrict__ expected,
                                                       size_t stride, uint32_t* __restrict__ block_sizes,
                                                       uint64_t* __restrict__ numbers, uint32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) int32_t stage_all[256 * kStage];
  __shared__ uint32_t mism[256];
  const uint32_t per_block = blockDim.x / channels;  // frames never straddle workgroups
  const uint32_t lf = threadIdx.x / channels, c = threadIdx.x % channels;
  const uint32_t f = blockIdx.x * per_block + lf;
  const bool live = f < n_frames && lf < per_block;
  mism[threadIdx.x] = 0;
  __syncthreads();
  uint32_t st = 1, bs = 0, ch_tag = 0, flen = 0, start = 0;
  if (live) {
    const FrameRec& r = recs[f];
    st = r.status;
    if (st == 0) {
      bs = r.block_size;
      ch_tag = (r.info >> 4) & 15u;
      flen = r.len;
      start = r.sub_bit[c];
    }
  }
  uint32_t order = 0;
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const uint8_t* fp = live ? bytes + offsets[f] : bytes;
  if (bs) {
    flacdec::BitReader r;
    r.init(fp, flen, start);
    flacdec::SubInfo si;
    flacdec::parse_subframe_header(r, bs, sbps, si);
    order = si.order;
  }
  const int bucket = flacdec::order_bucket(order);
  const size_t row0 = (static_cast<size_t>(f) * channels + c) * stride;
  int32_t* row = (!VERIFY && live) ? out + row0 : nullptr;
  const int32_t* erow = (VERIFY && live) ? expected + row0 : nullptr;
  int32_t* stage = stage_all + threadIdx.x * kStage;
  bool bad;
  if (__any(bucket == 32)) bad = run_subframe<32, VERIFY>(fp, flen, start, bs, sbps, ch_tag, c, row, erow, stage);
  else if (__any(bucket == 16)) bad = run_subframe<16, VERIFY>(fp, flen, start, bs, sbps, ch_tag, c, row, erow, stage);
  else if (__any(bucket == 8)) bad = run_subframe<8, VERIFY>(fp, flen, start, bs, sbps, ch_tag, c, row, erow, stage);
  else bad = run_subframe<4, VERIFY>(fp, flen, start, bs, sbps, ch_tag, c, row, erow, stage);
  if (!VERIFY && live)
    for (uint32_t t = bs; t < max_block_size; ++t) row[t] = 0;  // the rest of the row; all of it for a bad frame
  if (bad) atomicOr(&mism[lf], flacdec::MISMATCH);
  __syncthreads();
  if (live && c == 0) {
    const uint32_t s = st | mism[lf];
    status[f] = s;
    if (block_sizes) block_sizes[f] = s ? 0 : bs;
    if (numbers) numbers[f] = s ? 0 : nums[f];
  }
}

// ---------------------------------------------------------------- index
constexpr uint32_t kPosPerThread = 16, kPosPerBlock = 256 * kPosPerThread;

__device__ bool is_candidate(const uint8_t* bytes, uint64_t n_bytes, uint64_t p, uint32_t channels, uint32_t bps) {
  if (p + 1 >= n_bytes || bytes[p] != 0xFFu || (bytes[p + 1] & 0xFEu) != 0xF8u) return false;
  const uint64_t left = n_bytes - p;
  flacdec::Header h;
  return flacdec::parse_header(bytes + p, left > 64 ? 64u : static_cast<uint32_t>(left), channels, bps, 65536u, kCrc,
                               h) == 0;
}

__device__ uint32_t thread_candidates(const uint8_t* bytes, uint64_t n_bytes, uint64_t base, uint32_t channels,
                                      uint32_t bps, uint32_t* mask) {
  uint32_t m = 0;
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if (is_candidate(bytes, n_bytes, base + k, channels, bps)) m |= 1u << k;
  *mask = m;
  return __popc(m);
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

__global__ void __launch_bounds__(256) cand_count_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                         uint32_t channels, uint32_t bps,
                                                         uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t sh[256];
  uint32_t mask, total;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock + threadIdx.x * kPosPerThread;
  block_scan(thread_candidates(bytes, n_bytes, base, channels, bps, &mask), sh, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one workgroup: block_counts -> exclusive offsets in place; counters[0] = the number of candidates
__global__ void __launch_bounds__(1024) cand_scan_kernel(uint32_t* __restrict__ block_counts, uint32_t n_blocks,
                                                         uint32_t* __restrict__ counters) {
  __shared__ uint32_t sh[1024];
  const uint32_t per = (n_blocks + 1023) / 1024;
  const uint32_t lo = min(n_blocks, threadIdx.x * per), hi = min(n_blocks, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += block_counts[i];
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t x = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  uint32_t run = sh[threadIdx.x] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t v = block_counts[i];
    block_counts[i] = run;
    run += v;
  }
  if (threadIdx.x == 1023) counters[0] = sh[1023];
}

__global__ void __launch_bounds__(256) cand_write_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                         uint32_t channels, uint32_t bps,
                                                         const uint32_t* __restrict__ block_offsets,
                                                         uint64_t* __restrict__ cand_pos, uint32_t capacity) {
  __shared__ uint32_t sh[256];
  uint32_t mask, total;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock + threadIdx.x * kPosPerThread;
  uint32_t at = block_offsets[blockIdx.x] + block_scan(thread_candidates(bytes, n_bytes, base, channels, bps, &mask),
                                                       sh, &total);
  for (uint32_t k = 0; k < kPosPerThread; ++k)
    if ((mask >> k) & 1u) {
      if (at < capacity) cand_pos[at] = base + k;
      ++at;
    }
}

// jump[0][i]: the valid candidate (skim and CRC-16 passed) that starts where candidate i ends, kEnd at n_bytes, kDead
// otherwise -- so a chain only ever walks over verified frames, also when candidates were dropped at `capacity`
__global__ void __launch_bounds__(256) link_kernel(const uint64_t* __restrict__ cand_pos,
                                                   const FrameRec* __restrict__ recs, const uint32_t* __restrict__ n_dev,
                                                   uint32_t capacity, uint64_t n_bytes, uint32_t* __restrict__ jump) {
  const uint32_t n = min(*n_dev, capacity);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = kDead;
  if (recs[i].status == 0) {
    const uint64_t e = cand_pos[i] + recs[i].len;
    if (e == n_bytes) {
      nx = kEnd;
    } else {
      uint32_t lo = i + 1, hi = n;  // positions ascend
      while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (cand_pos[mid] < e) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n && cand_pos[lo] == e && recs[lo].status == 0) nx = lo;
    }
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

// one thread: the length of the chain from candidate 0 by binary lifting over the jump levels
__global__ void chain_kernel(const uint64_t* __restrict__ cand_pos, const FrameRec* __restrict__ recs,
                             const uint32_t* __restrict__ jump, uint32_t levels, uint32_t* __restrict__ counters,
                             uint32_t capacity, uint64_t n_bytes, uint64_t max_frames,
                             uint64_t* __restrict__ n_frames) {
  const uint32_t total = counters[0], n = min(total, capacity);
  // candidates past `capacity` (the highest positions) were dropped: what the chain reaches is still a verified
  // prefix, but it may stop early, so the caller is told to come back with a larger max_frames
  uint64_t err = total > capacity ? kIndexError : 0;
  uint64_t count = 0;
  if (n_bytes == 0) {
    // an empty buffer holds no frame and no error
  } else if (n == 0 || cand_pos[0] != 0 || recs[0].status != 0) {
    err = kIndexError;  // no verified frame at byte 0
  } else {
    uint32_t cur = 0;
    count = 1;
    for (int k = static_cast<int>(levels) - 1; k >= 0; --k) {
      const uint32_t nx = jump[static_cast<size_t>(k) * capacity + cur];
      if (nx < kEnd) {
        cur = nx;
        count += 1ull << k;
      }
    }
    if (jump[cur] != kEnd) err = kIndexError;
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
  uint32_t node = 0;
  for (uint32_t k = 0; k < levels; ++k)
    if ((m >> k) & 1u) node = jump[static_cast<size_t>(k) * capacity + node];
  offsets[m] = cand_pos[node];
  lengths[m] = recs[node].len;
}

uint32_t jump_levels(size_t capacity) {
  uint32_t l = 1;
  while ((static_cast<size_t>(1) << l) <= capacity) ++l;
  return l;
}

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

}  // namespace

size_t decode_scratch_bytes(size_t n_frames) { return align256(n_frames * sizeof(FrameRec)) + n_frames * 8; }

hipError_t launch_decode_frames(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                                const uint32_t* lengths, uint32_t n_frames, uint32_t channels, uint32_t bps,
                                uint32_t max_block_size, int32_t* out, const int32_t* expected, size_t stride,
                                uint32_t* block_sizes, uint64_t* numbers, uint32_t* status, void* scratch,
                                hipStream_t stream) {
  FrameRec* recs = static_cast<FrameRec*>(scratch);
  uint64_t* nums = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + align256(n_frames * sizeof(FrameRec)));
  hipLaunchKernelGGL(skim_kernel, dim3(ceil_div(n_frames, 256)), dim3(256), 0, stream, bytes, n_bytes, offsets,
                     lengths, n_frames, nullptr, channels, bps, max_block_size, recs, nums);
  hipLaunchKernelGGL(crc16_kernel, dim3(ceil_div(n_frames, 4)), dim3(256), 0, stream, bytes, offsets, n_frames,
                     nullptr, recs);
  const uint32_t per_block = 256 / channels;
  const dim3 grid(ceil_div(n_frames, per_block)), block(per_block * channels);
  if (expected)
    hipLaunchKernelGGL(subframe_kernel<true>, grid, block, 0, stream, bytes, offsets, recs, nums, n_frames, channels,
                       bps, max_block_size, nullptr, expected, stride, nullptr, nullptr, status);
  else
    hipLaunchKernelGGL(subframe_kernel<false>, grid, block, 0, stream, bytes, offsets, recs, nums, n_frames, channels,
                       bps, max_block_size, out, nullptr, stride, block_sizes, numbers, status);
  return hipGetLastError();
}

// what the batch index (flac_decode_streams.cpp) shares with this one: neither kernel looks at stream parameters
hipError_t launch_frame_crc16(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const uint32_t* n_dev,
                              void* recs, hipStream_t stream) {
  hipLaunchKernelGGL(crc16_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, stream, bytes, offsets, n, n_dev,
                     static_cast<FrameRec*>(recs));
  return hipGetLastError();
}

hipError_t launch_jump_levels(uint32_t* jump, const uint32_t* n_dev, size_t capacity, hipStream_t stream) {
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = jump_levels(capacity);
  for (uint32_t k = 1; k < levels; ++k)
    hipLaunchKernelGGL(jump_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, stream,
                       jump + static_cast<size_t>(k - 1) * cap, jump + static_cast<size_t>(k) * cap, n_dev, cap);
  return hipGetLastError();
}

uint32_t index_jump_levels(size_t capacity) { return jump_levels(capacity); }

size_t index_candidate_capacity(size_t max_frames) { return max_frames + max_frames / 4 + 4096; }

size_t index_scratch_bytes(uint64_t n_bytes, size_t capacity) {
  const size_t n_blocks = (n_bytes + kPosPerBlock - 1) / kPosPerBlock;
  return align256(n_blocks * 4) + 256 + align256(capacity * 8) + align256(capacity * sizeof(FrameRec)) +
         static_cast<size_t>(jump_levels(capacity)) * capacity * 4;
}

hipError_t launch_index_frames(const uint8_t* bytes, uint64_t n_bytes, uint32_t channels, uint32_t bps,
                               size_t max_frames, uint64_t* offsets, uint32_t* lengths, uint64_t* n_frames,
                               void* scratch, size_t capacity, hipStream_t stream) {
  const uint32_t n_blocks = ceil_div(n_bytes, kPosPerBlock);
  const uint32_t cap = static_cast<uint32_t>(capacity), levels = jump_levels(capacity);
  char* s = static_cast<char*>(scratch);
  uint32_t* block_counts = reinterpret_cast<uint32_t*>(s);
  s += align256(static_cast<size_t>(n_blocks) * 4);
  uint32_t* counters = reinterpret_cast<uint32_t*>(s);
  s += 256;
  uint64_t* cand_pos = reinterpret_cast<uint64_t*>(s);
  s += align256(capacity * 8);
  FrameRec* recs = reinterpret_cast<FrameRec*>(s);
  s += align256(capacity * sizeof(FrameRec));
  uint32_t* jump = reinterpret_cast<uint32_t*>(s);
  hipError_t e = hipMemsetAsync(counters, 0, 256, stream);
  if (e != hipSuccess) return e;
  if (n_blocks) {
    hipLaunchKernelGGL(cand_count_kernel, dim3(n_blocks), dim3(256), 0, stream, bytes, n_bytes, channels, bps,
                       block_counts);
    hipLaunchKernelGGL(cand_scan_kernel, dim3(1), dim3(1024), 0, stream, block_counts, n_blocks, counters);
    hipLaunchKernelGGL(cand_write_kernel, dim3(n_blocks), dim3(256), 0, stream, bytes, n_bytes, channels, bps,
                       block_counts, cand_pos, cap);
    hipLaunchKernelGGL(skim_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, stream, bytes, n_bytes, cand_pos,
                       nullptr, cap, counters, channels, bps, 65536u, recs, nullptr);
    hipLaunchKernelGGL(crc16_kernel, dim3(ceil_div(cap, 4)), dim3(256), 0, stream, bytes, cand_pos, cap, counters,
                       recs);
    hipLaunchKernelGGL(link_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, stream, cand_pos, recs, counters, cap,
                       n_bytes, jump);
    for (uint32_t k = 1; k < levels; ++k)
      hipLaunchKernelGGL(jump_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, stream,
                         jump + static_cast<size_t>(k - 1) * cap, jump + static_cast<size_t>(k) * cap, counters, cap);
  }
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(1), 0, stream, cand_pos, recs, jump, levels, counters, cap,
                     n_bytes, static_cast<uint64_t>(max_frames), n_frames);
  if (max_frames)
    hipLaunchKernelGGL(enumerate_kernel, dim3(ceil_div(max_frames < cap ? max_frames : cap, 256)), dim3(256), 0,
                       stream, cand_pos, recs, jump, levels, counters, cap, offsets, lengths);
  return hipGetLastError();
}

}  // namespace flacenc_hip
