// pcm_pack.cpp -- the kernels of flacenc_hip_pack_le_bytes: decoded rows (channel-major int32, one block size per frame)
// to packed interleaved little-endian PCM, the inverse of fill_le_bytes_kernel.  Index arithmetic: pcm_pack_core.h.
#include "pcm_pack.h"

#include "pcm_pack_core.h"

namespace flacenc_hip {

namespace {

// Exclusive prefix sum of the clamped block sizes, frame_offsets_kernel's scan: one workgroup walks the frames 1024 at a
// time and carries the running sum, so any frame count is one launch (8 steps for a group of the stream decoder).
__global__ __launch_bounds__(1024) void pcm_offsets_kernel(const uint32_t* __restrict__ block_sizes,
                                                            unsigned long long n, uint32_t clamp,
                                                            uint64_t* __restrict__ offsets,
                                                            uint64_t* __restrict__ total) {
  __shared__ unsigned long long wave_sums[16];
  __shared__ unsigned long long carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (unsigned long long base = 0; base < n; base += 1024u) {
    const unsigned long long f = base + tid;
    unsigned long long v = 0;
    if (f < n) {
      const uint32_t b = block_sizes[f];
      v = b < clamp ? b : clamp;
    }
    unsigned long long s = v;  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(s, d, 64);
      if ((int)lane >= d) s += o;
    }
    if (lane == 63) wave_sums[wave] = s;
    __syncthreads();
    unsigned long long before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += wave_sums[w];
    if (f < n) offsets[f] = before + s - v;
    __syncthreads();
    if (tid == 1023) carry = before + s;
    __syncthreads();
  }
  if (tid == 0) {
    offsets[n] = carry;
    total[0] = carry;
  }
}

// A workgroup per (frame, slice of pcmpack::SLICE samples), grid-stride over frames x slices so that the frame count
// is not bound by a grid dimension.  Output dword k of the slice's span is assembled in registers from the (at most
// four) samples whose bytes it holds: for a fixed channel consecutive lanes read consecutive samples of one row, and the
// stores are destination-aligned dwords, as in place_frames_kernel.  The span's head and tail bytes share their dword with
// the neighbouring span (another workgroup, another frame or slice): byte stores, never a read-modify-write.
template <int B>
__global__ __launch_bounds__(256) void pack_le_bytes_kernel(const int32_t* __restrict__ frames,
                                                            unsigned long long stride,
                                                            const uint32_t* __restrict__ block_sizes,
                                                            const uint64_t* __restrict__ offsets,
                                                            unsigned long long n_frames, uint32_t channels,
                                                            uint32_t magic, unsigned long long spf,
                                                            uint8_t* __restrict__ out,
                                                            unsigned long long out_capacity) {
  if (offsets[n_frames] * channels * B > out_capacity) return;  // no room: nothing is written
  const uint32_t clamp = stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(stride);
  const unsigned long long work = n_frames * spf;
  for (unsigned long long w = blockIdx.x; w < work; w += gridDim.x) {
    const unsigned long long f = w / spf, sl = w - f * spf;
    uint32_t bs = block_sizes[f];
    if (bs > clamp) bs = clamp;
    const uint32_t ns = pcmpack::slice_samples(bs, sl);
    if (ns == 0) continue;
    const unsigned long long s0 = sl * pcmpack::SLICE;
    const int32_t* rows = frames + f * channels * stride + s0;
    auto load = [&](uint32_t c, uint32_t i) { return rows[c * stride + i]; };
    uint8_t* d = out + (offsets[f] + s0) * channels * B;
    const uint32_t len = ns * channels * B;
    const pcmpack::Split sp = pcmpack::split(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d)), len);
    if (threadIdx.x < sp.head) d[threadIdx.x] = static_cast<uint8_t>(pcmpack::byte_at<B>(threadIdx.x, channels, magic, load));
    uint32_t* dw = reinterpret_cast<uint32_t*>(d + sp.head);
    for (uint32_t k = threadIdx.x; k < sp.n_dwords; k += 256u)
      dw[k] = pcmpack::dword_at<B>(sp.head + 4u * k, channels, magic, load);
    const uint32_t t0 = sp.head + 4u * sp.n_dwords;
    if (threadIdx.x < sp.tail)
      d[t0 + threadIdx.x] = static_cast<uint8_t>(pcmpack::byte_at<B>(t0 + threadIdx.x, channels, magic, load));
  }
}

}  // namespace

hipError_t launch_pcm_offsets(const uint32_t* block_sizes, uint64_t n_frames, size_t stride, uint64_t* offsets,
                              uint64_t* total, hipStream_t stream) {
  const uint32_t clamp = stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(stride);
  hipLaunchKernelGGL(pcm_offsets_kernel, dim3(1), dim3(1024), 0, stream, block_sizes,
                     static_cast<unsigned long long>(n_frames), clamp, offsets, total);
  return hipGetLastError();
}

hipError_t launch_pack_le_bytes(const int32_t* frames, size_t stride, const uint32_t* block_sizes,
                                const uint64_t* offsets, uint64_t n_frames, uint32_t channels,
                                uint32_t bytes_per_sample, uint8_t* out, uint64_t out_capacity, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  const unsigned long long spf = pcmpack::slices_per_frame(stride);
  const unsigned long long work = n_frames * spf;
  const uint32_t grid = work < (1ull << 20) ? static_cast<uint32_t>(work) : (1u << 20);
  const uint32_t magic = pcmpack::div_magic(channels);
#define PPK_LAUNCH(B)                                                                                              \
  hipLaunchKernelGGL(pack_le_bytes_kernel<B>, dim3(grid), dim3(256), 0, stream, frames,                            \
                     static_cast<unsigned long long>(stride), block_sizes, offsets,                                \
                     static_cast<unsigned long long>(n_frames), channels, magic, spf, out,                         \
                     static_cast<unsigned long long>(out_capacity))
  switch (bytes_per_sample) {
    case 1: PPK_LAUNCH(1); break;
    case 2: PPK_LAUNCH(2); break;
    case 3: PPK_LAUNCH(3); break;
    case 4: PPK_LAUNCH(4); break;
    default: return hipErrorInvalidValue;
  }
#undef PPK_LAUNCH
  return hipGetLastError();
}

}  // namespace flacenc_hip
