// encode_streams_planar.cpp -- flacenc_hip_encode_streams_planar: a batch of planar int32 / float32 rows, a [B, C, T]
// tensor as it lies, to FLAC frames in one call.  The call is flacenc_hip_encode_streams with
// another source: the plan, the runs, the scan, the cut and the place are encode_streams.cpp's, this file holds what
// touches the elements:
//   planar_fill_kernel   the rows of a table of frames into the 16-byte aligned channel-major int32 rows the frame-level
//                        calls take, float32 quantised on the way (planarenc::quantise), zero beyond the frame's samples;
//                        counts the elements that clamped or were NaN
//   planar_pack_kernel   only where digests are asked for: every stream's packed interleaved little-endian PCM, once,
//                        with dword stores, for md5_spans_kernel to hash
// No element outside [0, total_samples) of a stream's rows is read by either.
#include "api_internal.h"
#include "stream_planar_encode_core.h"

namespace flacenc_hip {
namespace {

using planarenc::Frame;
using planarenc::Stream;
using Desc = flacenc_hip_pcm_stream_desc;

static_assert(sizeof(Frame) == 32 && sizeof(Stream) == 32, "table layouts");

// One lane: four sample times of one frame, all channels: per channel four elements in, one 16-byte store out.  The work
// items (frame, group of four sample times) are numbered flat as in streams_fill_kernel; the loop is uniform across the
// wave (a lane behind the last item idles through it), so that the clip counts can be summed across the wave.
//   FORM 1  two aligned 16-byte loads brought into place, where all eight elements lie inside the frame's row (an
//           aligned row: one load); the frame's first and last groups go the dword way.  What the product runs: the
//           faster of the two
//   FORM 0  the four elements as four dword loads: neighbouring lanes read neighbouring 16 bytes
// Clip counting costs a compare and a lane-local add per element; only a wave in which some lane counted reduces (per
// stream: a wave can span frames of several) and issues one atomic per stream.
template <int C, int F32, int FORM>
__global__ void __launch_bounds__(256) planar_fill_kernel(const uint32_t* __restrict__ elems,
                                                          const Frame* __restrict__ table, uint32_t n_frames,
                                                          uint32_t row0, uint32_t groups, size_t stride, uint32_t bits,
                                                          int32_t* __restrict__ rows,
                                                          unsigned long long* __restrict__ clipped) {
  const uint64_t items = static_cast<uint64_t>(n_frames) * groups;
  const bool narrow = items <= 0xFFFFFFFFull;
  const float scale = planarenc::scale_of(bits);
  const int32_t hi = static_cast<int32_t>(1u << (bits - 1));  // (read for float32 elements alone: bits <= 24)
  for (uint64_t base = blockIdx.x * 256ull; base < items; base += static_cast<uint64_t>(gridDim.x) * 256ull) {
    const uint64_t it = base + threadIdx.x;
    uint32_t cnt = 0, stream = 0;
    if (it < items) {
      const uint32_t f = narrow ? static_cast<uint32_t>(it) / groups : static_cast<uint32_t>(it / groups);
      const uint32_t t0 = static_cast<uint32_t>(it - static_cast<uint64_t>(f) * groups) * 4u;
      const Frame fr = table[f];
      stream = fr.stream;
      const uint32_t n = t0 < fr.valid ? (fr.valid - t0 < 4u ? fr.valid - t0 : 4u) : 0u;
      int32_t* dst = rows + (static_cast<size_t>(row0) + f) * C * stride + t0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t* p = elems + fr.elem0 + static_cast<uint64_t>(c) * fr.pitch + t0;
        uint32_t e[4] = {0, 0, 0, 0};
        const uint32_t lead = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
        if (FORM == 1 && n == 4 && lead == 0) {
          const uint4 a = *reinterpret_cast<const uint4*>(p);
          e[0] = a.x, e[1] = a.y, e[2] = a.z, e[3] = a.w;
        } else if (FORM == 1 && n == 4 && t0 >= lead && t0 - lead + 8u <= fr.valid) {
          const uint4 a = *reinterpret_cast<const uint4*>(p - lead);
          const uint4 b = *reinterpret_cast<const uint4*>(p - lead + 4);
          e[0] = lead == 1 ? a.y : lead == 2 ? a.z : a.w;
          e[1] = lead == 1 ? a.z : lead == 2 ? a.w : b.x;
          e[2] = lead == 1 ? a.w : lead == 2 ? b.x : b.y;
          e[3] = lead == 1 ? b.x : lead == 2 ? b.y : b.z;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (static_cast<uint32_t>(j) < n) e[j] = p[j];
        }
        int4 v;
        if (F32) {
          v.x = planarenc::quantise(planarenc::as_float(e[0]), scale, hi, &cnt);
          v.y = planarenc::quantise(planarenc::as_float(e[1]), scale, hi, &cnt);
          v.z = planarenc::quantise(planarenc::as_float(e[2]), scale, hi, &cnt);
          v.w = planarenc::quantise(planarenc::as_float(e[3]), scale, hi, &cnt);
        } else {
          v.x = static_cast<int32_t>(e[0]), v.y = static_cast<int32_t>(e[1]);
          v.z = static_cast<int32_t>(e[2]), v.w = static_cast<int32_t>(e[3]);
        }
        *reinterpret_cast<int4*>(dst + static_cast<size_t>(c) * stride) = v;
      }
    }
    if (F32 && clipped) {
      unsigned long long pending = __ballot(cnt != 0);
      while (pending) {  // rare: one round per stream with a count in this wave
        const int leader = __ffsll(pending) - 1;
        const uint32_t ls = __shfl(stream, leader, 64);
        const bool mine = cnt != 0 && stream == ls;
        uint32_t sum = mine ? cnt : 0u;
#pragma unroll
        for (int m = 32; m; m >>= 1) sum += __shfl_xor(sum, m, 64);
        if (static_cast<int>(threadIdx.x & 63u) == leader) atomicAdd(clipped + ls, static_cast<unsigned long long>(sum));
        pending &= ~__ballot(mine);
      }
    }
  }
}

// One lane: one dword of one stream's packed PCM, of the dwords whose first byte lies in one frame's samples (so every
// dword of a stream belongs to exactly one frame of the table and the kernel walks the table the fills walk).  Channels
// and bytes per sample are read per frame: one launch serves every class.  A stream's last dword is filled up with zero
// inside the slack its slot has behind it.
template <int F32>
__global__ void __launch_bounds__(256) planar_pack_kernel(const uint32_t* __restrict__ elems,
                                                          const Frame* __restrict__ table, uint32_t n_frames,
                                                          const Stream* __restrict__ streams,
                                                          const Desc* __restrict__ descs, uint32_t per,
                                                          uint8_t* __restrict__ image) {
  const uint64_t items = static_cast<uint64_t>(n_frames) * per;
  for (uint64_t it = blockIdx.x * 256ull + threadIdx.x; it < items; it += static_cast<uint64_t>(gridDim.x) * 256ull) {
    const uint32_t f = static_cast<uint32_t>(it / per);
    const uint32_t j = static_cast<uint32_t>(it - static_cast<uint64_t>(f) * per);
    const Frame fr = table[f];
    const uint32_t C = descs[fr.stream].channels, B = descs[fr.stream].bytes_per_sample, bits = descs[fr.stream].bits_per_sample;
    const Stream st = streams[fr.stream];
    const uint64_t lo = fr.first * C * B, hi = lo + static_cast<uint64_t>(fr.valid) * C * B;
    const uint64_t k0 = ((lo + 3u) / 4u + j) * 4u;
    if (k0 >= hi) continue;
    const uint64_t end = st.total_samples * C * B;
    const float scale = planarenc::scale_of(bits);
    const int32_t top = static_cast<int32_t>(1u << (bits - 1));  // (read for float32 elements alone: bits <= 24)
    planarenc::PackedByte at = planarenc::packed_byte(k0, C, B);
    uint32_t word = 0, unused = 0;
    int32_t v = 0;
    bool have = false;
    for (uint32_t b = 0; b < 4 && k0 + b < end; ++b) {
      if (!have) {
        const uint32_t e = elems[st.elem0 + static_cast<uint64_t>(at.c) * st.pitch + at.t];
        v = planarenc::sample_of(e, F32 ? FLACENC_HIP_SAMPLE_F32 : FLACENC_HIP_SAMPLE_I32, scale, top, &unused);
        have = true;
      }
      word |= ((static_cast<uint32_t>(v) >> (8u * at.b)) & 0xFFu) << (8u * b);
      if (++at.b == B) {
        at.b = 0;
        have = false;
        if (++at.c == C) {
          at.c = 0;
          ++at.t;
        }
      }
    }
    *reinterpret_cast<uint32_t*>(image + st.packed_base + k0) = word;
  }
}

template <int C, int F32>
hipError_t launch_fill_cf(int form, dim3 grid, hipStream_t st, const uint32_t* elems, const Frame* table, uint32_t n_frames,
                          uint32_t row0, uint32_t groups, size_t stride, uint32_t bits, int32_t* rows,
                          unsigned long long* clipped) {
  if (form == 1)
    hipLaunchKernelGGL((planar_fill_kernel<C, F32, 1>), grid, dim3(256), 0, st, elems, table, n_frames, row0, groups, stride, bits, rows, clipped);
  else
    hipLaunchKernelGGL((planar_fill_kernel<C, F32, 0>), grid, dim3(256), 0, st, elems, table, n_frames, row0, groups, stride, bits, rows, clipped);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_planar_fill(const uint32_t* elems, const Frame* table, uint32_t n_frames, uint32_t channels,
                              uint32_t sample_format, uint32_t bits, uint32_t row0, size_t stride, int32_t* rows,
                              unsigned long long* clipped, int form, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  if (bits < 1 || bits > (sample_format == FLACENC_HIP_SAMPLE_I32 ? 32u : 24u)) return hipErrorInvalidValue;
  const uint32_t groups = static_cast<uint32_t>(stride / 4);
  const uint64_t items = static_cast<uint64_t>(n_frames) * groups;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((items + 255) / 256, 65536)));
#define PF_FILL(C)                                                                                                        \
  case C:                                                                                                                 \
    return sample_format == FLACENC_HIP_SAMPLE_F32                                                                        \
               ? launch_fill_cf<C, 1>(form, grid, stream, elems, table, n_frames, row0, groups, stride, bits, rows, clipped) \
               : launch_fill_cf<C, 0>(form, grid, stream, elems, table, n_frames, row0, groups, stride, bits, rows, clipped)
  switch (channels) {
    PF_FILL(1);
    PF_FILL(2);
    PF_FILL(3);
    PF_FILL(4);
    PF_FILL(5);
    PF_FILL(6);
    PF_FILL(7);
    PF_FILL(8);
  }
#undef PF_FILL
  return hipErrorInvalidValue;
}

hipError_t launch_planar_pack(const uint32_t* elems, const Frame* table, uint32_t n_frames, const Stream* streams,
                              const Desc* descs, uint32_t per, uint32_t sample_format, uint8_t* image, hipStream_t stream) {
  if (n_frames == 0 || per == 0) return hipSuccess;
  const uint64_t items = static_cast<uint64_t>(n_frames) * per;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((items + 255) / 256, 65536)));
  if (sample_format == FLACENC_HIP_SAMPLE_F32)
    hipLaunchKernelGGL(planar_pack_kernel<1>, grid, dim3(256), 0, stream, elems, table, n_frames, streams, descs, per, image);
  else
    hipLaunchKernelGGL(planar_pack_kernel<0>, grid, dim3(256), 0, stream, elems, table, n_frames, streams, descs, per, image);
  return hipGetLastError();
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" int flacenc_hip_encode_streams_planar(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                                 const void* samples, uint64_t samples_bytes, uint32_t sample_format,
                                                 uint64_t row_pitch, const void* streams, size_t n_streams,
                                                 uint32_t block_size, uint8_t* out, uint64_t out_bytes,
                                                 uint32_t* frame_lengths, size_t max_frames, uint64_t* totals,
                                                 uint64_t call_totals[2], uint8_t* digests, uint64_t* clipped,
                                                 int memory_kind) {
  const PlanarSource src = {samples, samples_bytes, sample_format, row_pitch, digests, clipped};
  return encode_streams_common(h, cfg, nullptr, 0, &src, streams, n_streams, block_size, out, out_bytes, frame_lengths,
                               max_frames, totals, call_totals, memory_kind);
}
