// variable_block.cpp -- the block-size search's own kernels (flacenc_hip_encode_variable_async).  Each candidate block
// is coded by the fixed-blocking encode+pack call at its block size (the frame bodies are pinned by construction); the
// kernels here are launch- and bandwidth-shaped: they move samples into the levels' frames, choose each superblock's
// tiling by a tree minimum over the packed lengths, and rewrite the chosen frames' headers without reading their bodies
// twice (the CRC-16 is combined, variable_block_core.h).
#include "variable_block.h"

#include "flacenc_hip.h"
#include "variable_block_core.h"

namespace flacenc_hip {
namespace {

// Level k of the search: every superblock's channel rows cut into 2^k rows of b = S >> k samples.  vec: 16-byte moves
// (b, both strides and both bases multiples of 4 samples / 16 bytes), else one sample per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void reblock_kernel(const int32_t* __restrict__ src, size_t src_stride,
                                                      uint32_t n_full, uint32_t channels, uint32_t superblock,
                                                      uint32_t level, int32_t* __restrict__ dst, size_t dst_stride) {
  const uint32_t b = superblock >> level;
  const uint32_t per_row = VEC ? b / 4u : b;
  const uint64_t rows = (uint64_t)n_full * channels << level;
  const uint64_t total = rows * per_row;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256u) {
    const uint64_t row = t / per_row;
    const uint32_t q = (uint32_t)(t - row * per_row);
    const uint64_t f = row / channels;
    const uint32_t c = (uint32_t)(row - f * channels);
    const uint64_t i = f >> level;
    const uint32_t j = (uint32_t)(f & ((1u << level) - 1u));
    const int32_t* s = src + (i * channels + c) * src_stride + (size_t)j * b;
    int32_t* d = dst + row * dst_stride;
    if (VEC) reinterpret_cast<int4*>(d)[q] = reinterpret_cast<const int4*>(s)[q];
    else d[q] = s[q];
  }
}

__device__ __forceinline__ uint32_t sb_levels(const VbsLayout& l, uint32_t i) { return i < l.n_full ? l.levels : 1u; }
__device__ __forceinline__ uint32_t sb_block(const VbsLayout& l, uint32_t i, uint32_t k) {
  return i < l.n_full ? (l.superblock >> k) : l.tail;
}

// heap node n of superblock i: its level, frame index inside the level, block size and sample number
struct Node {
  uint32_t level, index, block;
  uint64_t sample;
};
__device__ __forceinline__ Node node_of(const VbsLayout& l, uint32_t i, uint32_t n) {
  Node r;
  r.level = vbs::node_level(n);
  const uint32_t j = n - (1u << r.level);
  r.index = (i << r.level) + j;
  r.block = sb_block(l, i, r.level);
  r.sample = l.first_sample + (uint64_t)i * l.superblock + (uint64_t)j * r.block;
  return r;
}
__device__ __forceinline__ uint32_t node_length(const VbsLayout& l, const Node& n) {
  return vbs::variable_length(l.lens[l.len_base[n.level] + n.index], n.index, n.sample);
}

__global__ __launch_bounds__(256) void vbs_decide_kernel(VbsLayout l, uint32_t* __restrict__ masks,
                                                         uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= l.n_full + (l.tail ? 1u : 0u)) return;
  const uint32_t levels = sb_levels(l, i);
  uint32_t len[vbs::MAX_NODES + 1];
  for (uint32_t n = 1; n < (1u << levels); ++n) len[n] = node_length(l, node_of(l, i, n));
  uint32_t mask, count;
  vbs::tree_min(len, levels, &mask, &count);
  masks[i] = mask;
  counts[i] = count;
}

__global__ __launch_bounds__(256) void vbs_emit_kernel(VbsLayout l, const uint32_t* __restrict__ masks,
                                                       const uint32_t* __restrict__ counts,
                                                       const uint64_t* __restrict__ first, uint32_t max_slots,
                                                       VbsChosen* __restrict__ chosen, uint32_t* __restrict__ vlen,
                                                       uint32_t* __restrict__ user_masks) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= l.n_full + (l.tail ? 1u : 0u)) return;
  const uint32_t levels = sb_levels(l, i), mask = masks[i], count = counts[i];
  const uint64_t f0 = first[i];
  for (uint32_t t = 0; t < count; ++t) {
    const uint64_t f = f0 + t;
    if (f >= max_slots) break;
    const Node n = node_of(l, i, vbs::tiling_node(mask, levels, t));
    VbsChosen c;
    c.sample = n.sample;
    c.level = n.level;
    c.index = n.index;
    c.block = n.block;
    c.pad = 0;
    chosen[f] = c;
    vlen[f] = node_length(l, n);
  }
  if (user_masks) user_masks[i] = mask;
}

__constant__ vbs::XPow8 kXPow8 = vbs::make_xpow8();

// A workgroup per chosen frame (grid-stride).  The body moves as place_frames_kernel moves frames: destination-aligned
// dword stores fed from two aligned source loads.  Wave 0 also writes the new header and the CRC-16, combined from the
// old one without reading the body: x^(8|B|) is the product of the XPOW8 entries of |B|'s set bits, one per lane, reduced
// across the wave -- so no lane runs a serial square-and-multiply while the others copy.
__global__ __launch_bounds__(256) void rehead_kernel(VbsLayout l, const VbsChosen* __restrict__ chosen,
                                                     const uint64_t* __restrict__ voff,
                                                     const uint64_t* __restrict__ frame_total,
                                                     const uint64_t* __restrict__ byte_total, uint32_t max_slots,
                                                     uint8_t* __restrict__ out, uint64_t out_capacity,
                                                     uint64_t* __restrict__ frame_offsets,
                                                     uint32_t* __restrict__ frame_lengths,
                                                     uint32_t* __restrict__ frame_block_sizes, uint64_t max_frames,
                                                     uint64_t* __restrict__ totals) {
  const uint64_t nf = frame_total[0], nb = byte_total[0];
  const bool overflow = nf > max_frames || nb > out_capacity || nf > max_slots;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = nf | (overflow ? FLACENC_HIP_VARIABLE_OVERFLOW : 0ull);
    totals[1] = nb;
  }
  if (overflow) return;
  for (uint32_t f = blockIdx.x; f < nf; f += gridDim.x) {
    const VbsChosen c = chosen[f];
    const uint8_t* src = l.pack + l.pack_base[c.level] + (uint64_t)c.index * l.pack_stride[c.level];
    const uint32_t flen = l.lens[l.len_base[c.level] + c.index];
    uint8_t* dst = out + voff[f];
    const uint32_t hf = vbs::header_bytes(src);
    // (the frame must take exactly the bytes the scan gave it: a header that disagrees is not written at all)
    if (hf == 0 || flen < hf + 2u) continue;
    const uint32_t hv = hf - vbs::coded_number_bytes(c.index) + vbs::coded_number_bytes(c.sample);
    if (flen - hf + hv != vbs::variable_length(flen, c.index, c.sample)) continue;
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
        uint8_t h[16];
        vbs::write_variable_header(src, c.sample, h);
        for (uint32_t k = 0; k < hv; ++k) dst[k] = h[k];
        const uint32_t crc_old = ((uint32_t)src[flen - 2] << 8) | src[flen - 1];
        const uint32_t crc = vbs::crc16_combine(crc_old, vbs::crc16_bytes(src, hf), vbs::crc16_bytes(h, hv), p);
        dst[hv + body] = static_cast<uint8_t>(crc >> 8);
        dst[hv + body + 1] = static_cast<uint8_t>(crc);
        frame_offsets[f] = voff[f];
        frame_lengths[f] = hv + body + 2u;
        frame_block_sizes[f] = c.block;
      }
    }
  }
}

}  // namespace

hipError_t launch_reblock(const int32_t* src, size_t src_stride, uint32_t n_full, uint32_t channels,
                          uint32_t superblock, uint32_t level, int32_t* dst, size_t dst_stride, hipStream_t stream) {
  const uint32_t b = superblock >> level;
  const bool vec = b % 4u == 0u && src_stride % 4u == 0u && dst_stride % 4u == 0u &&
                   (reinterpret_cast<uintptr_t>(src) & 15u) == 0u && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u;
  const uint64_t total = ((uint64_t)n_full * channels << level) * (vec ? b / 4u : b);
  if (total == 0) return hipSuccess;
  uint64_t grid = (total + 255u) / 256u;
  if (grid > 65536u) grid = 65536u;
  if (vec) hipLaunchKernelGGL(reblock_kernel<true>, dim3((uint32_t)grid), dim3(256), 0, stream, src, src_stride, n_full,
                              channels, superblock, level, dst, dst_stride);
  else hipLaunchKernelGGL(reblock_kernel<false>, dim3((uint32_t)grid), dim3(256), 0, stream, src, src_stride, n_full,
                          channels, superblock, level, dst, dst_stride);
  return hipGetLastError();
}

hipError_t launch_vbs_decide(const VbsLayout& l, uint32_t* masks, uint32_t* counts, hipStream_t stream) {
  const uint32_t n = l.n_full + (l.tail ? 1u : 0u);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vbs_decide_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, l, masks, counts);
  return hipGetLastError();
}

hipError_t launch_vbs_emit(const VbsLayout& l, const uint32_t* masks, const uint32_t* counts, const uint64_t* first,
                           uint32_t max_slots, VbsChosen* chosen, uint32_t* vlen, uint32_t* user_masks,
                           hipStream_t stream) {
  const uint32_t n = l.n_full + (l.tail ? 1u : 0u);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vbs_emit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, l, masks, counts, first, max_slots,
                     chosen, vlen, user_masks);
  return hipGetLastError();
}

hipError_t launch_rehead(const VbsLayout& l, const VbsChosen* chosen, const uint64_t* voff,
                         const uint64_t* frame_total, const uint64_t* byte_total, uint32_t max_slots, uint8_t* out,
                         uint64_t out_capacity, uint64_t* frame_offsets, uint32_t* frame_lengths,
                         uint32_t* frame_block_sizes, uint64_t max_frames, uint64_t* totals, hipStream_t stream) {
  const uint32_t grid = max_slots == 0 ? 1u : (max_slots < 65536u ? max_slots : 65536u);
  hipLaunchKernelGGL(rehead_kernel, dim3(grid), dim3(256), 0, stream, l, chosen, voff, frame_total, byte_total, max_slots,
                     out, out_capacity, frame_offsets, frame_lengths, frame_block_sizes, max_frames, totals);
  return hipGetLastError();
}

}  // namespace flacenc_hip
