// flac_decode.cpp -- decode and verify FLAC frames on the GPU (flacenc_hip_decode_frames and friends).
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
// The lane setup, the bucket ladder and the sample step are flac_decode_device.h's, shared with the packed-PCM decoders
// (flac_decode_streams.cpp, flac_decode_ranges.cpp).  The frame index -- flacenc_hip_index_frames included -- is
// stream_index.cpp; it runs crc16_kernel through launch_frame_crc16 and, for the single stream, skim_kernel in its
// index mode through launch_frame_skim.
#include "flac_decode.h"

#include "flac_decode_device.h"

namespace flacenc_hip {
namespace {

using flacdec::FrameRec;

__constant__ flacdec::CrcTables kCrc = flacdec::make_crc_tables();

constexpr int kStage = 20;  // LDS words per lane (16 staged samples, padded)

// ---------------------------------------------------------------- skim: one lane per frame
// index mode (lengths == NULL): frame i starts at offsets[i], may run to n_bytes, and its parsed length is recorded
__global__ void __launch_bounds__(256) skim_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                   const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lengths, uint32_t n,
                                                   const uint32_t* __restrict__ n_dev, uint32_t channels, uint32_t bps,
                                                   uint32_t max_block_size, uint32_t max_bps,
                                                   FrameRec* __restrict__ recs,
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
    flacdec::skim_frame(bytes + off, len, channels, bps, max_block_size, max_bps, lengths != nullptr, kCrc, rec, &num);
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
// WIDE, on: the decoder instance and the lane's flag (AT_WAVE_DECODER); a lane that is not on is idle
template <int MAXP, bool VERIFY, bool WIDE>
__device__ __forceinline__ bool run_subframe(const uint8_t* fp, uint32_t flen, uint32_t start, uint32_t bs, uint32_t sbps,
                             uint32_t ch_tag, uint32_t c, int32_t* row, const int32_t* erow, int32_t* stage, bool on) {
  if (!on) bs = 0;
  typename flacdec::Decoder<MAXP, WIDE>::type d;
  if (bs) d.init(fp, flen, start, bs, sbps);
  const int32_t* mem = VERIFY ? erow : row;
  const bool vec = (reinterpret_cast<uintptr_t>(mem) & 15u) == 0;
  bool bad = false;
  for (uint32_t t0 = 0; t0 < bs; t0 += 16) {
    const uint32_t m = min(16u, bs - t0);
    for (uint32_t i = 0; i < m; ++i) stage[i] = next_sample(d, ch_tag, c);
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

// DEEP: the launch's stream takes the wide decoder (AT_WAVE_DECODER; bps is the launch's, so every wave of a deep
// launch is wide)
template <bool VERIFY, bool DEEP>
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
  const uint32_t sbps = flacdec::subframe_bps(bps, ch_tag, c);
  const uint8_t* fp = live ? bytes + offsets[f] : bytes;
  const size_t row0 = (static_cast<size_t>(f) * channels + c) * stride;
  int32_t* row = (!VERIFY && live) ? out + row0 : nullptr;
  const int32_t* erow = (VERIFY && live) ? expected + row0 : nullptr;
  int32_t* stage = stage_all + threadIdx.x * kStage;
  const int bucket = lane_bucket(fp, flen, start, bs, sbps);
  bool bad = false;
  AT_WAVE_DECODER(DEEP, bucket, flacdec::needs_wide(bps),
                  bad |= run_subframe<MAXP, VERIFY, WIDE>(fp, flen, start, bs, sbps, ch_tag, c, row, erow, stage, ON));
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

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

}  // namespace

size_t decode_scratch_bytes(size_t n_frames) { return align256(n_frames * sizeof(FrameRec)) + n_frames * 8; }

hipError_t launch_decode_frames(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                                const uint32_t* lengths, uint32_t n_frames, uint32_t channels, uint32_t bps,
                                uint32_t max_block_size, uint32_t max_bps, int32_t* out, const int32_t* expected,
                                size_t stride, uint32_t* block_sizes, uint64_t* numbers, uint32_t* status,
                                void* scratch, hipStream_t stream) {
  FrameRec* recs = static_cast<FrameRec*>(scratch);
  uint64_t* nums = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + align256(n_frames * sizeof(FrameRec)));
  hipLaunchKernelGGL(skim_kernel, dim3(ceil_div(n_frames, 256)), dim3(256), 0, stream, bytes, n_bytes, offsets,
                     lengths, n_frames, nullptr, channels, bps, max_block_size, max_bps, recs, nums);
  hipLaunchKernelGGL(crc16_kernel, dim3(ceil_div(n_frames, 4)), dim3(256), 0, stream, bytes, offsets, n_frames,
                     nullptr, recs);
  const uint32_t per_block = 256 / channels;
  const dim3 grid(ceil_div(n_frames, per_block)), block(per_block * channels);
  const bool deep = flacdec::needs_wide(bps);
  if (expected && deep)
    hipLaunchKernelGGL((subframe_kernel<true, true>), grid, block, 0, stream, bytes, offsets, recs, nums, n_frames,
                       channels, bps, max_block_size, nullptr, expected, stride, nullptr, nullptr, status);
  else if (expected)
    hipLaunchKernelGGL((subframe_kernel<true, false>), grid, block, 0, stream, bytes, offsets, recs, nums, n_frames,
                       channels, bps, max_block_size, nullptr, expected, stride, nullptr, nullptr, status);
  else if (deep)
    hipLaunchKernelGGL((subframe_kernel<false, true>), grid, block, 0, stream, bytes, offsets, recs, nums, n_frames,
                       channels, bps, max_block_size, out, nullptr, stride, block_sizes, numbers, status);
  else
    hipLaunchKernelGGL((subframe_kernel<false, false>), grid, block, 0, stream, bytes, offsets, recs, nums, n_frames,
                       channels, bps, max_block_size, out, nullptr, stride, block_sizes, numbers, status);
  return hipGetLastError();
}

// skim_kernel in index mode and crc16_kernel for the frame index (stream_index.cpp)
hipError_t launch_frame_skim(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets, uint32_t n,
                             const uint32_t* n_dev, uint32_t channels, uint32_t bps, uint32_t max_bps, void* recs,
                             hipStream_t stream) {
  hipLaunchKernelGGL(skim_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, stream, bytes, n_bytes, offsets, nullptr, n, n_dev,
                     channels, bps, 65536u, max_bps, static_cast<FrameRec*>(recs), nullptr);
  return hipGetLastError();
}

hipError_t launch_frame_crc16(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const uint32_t* n_dev,
                              void* recs, hipStream_t stream) {
  hipLaunchKernelGGL(crc16_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, stream, bytes, offsets, n, n_dev,
                     static_cast<FrameRec*>(recs));
  return hipGetLastError();
}

}  // namespace flacenc_hip
