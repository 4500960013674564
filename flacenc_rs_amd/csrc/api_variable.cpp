// api_variable.cpp -- the block-size search's entry points (kernels: variable_block.cpp).
#include <algorithm>

#include "api_internal.h"
#include "variable_block.h"
#include "variable_block_core.h"

using namespace flacenc_hip;

namespace {
struct VbsShape {
  uint32_t n_full, tail;
  uint64_t n_sb, max_frames;
};

// superblock / level limits of the search; false with last_error set (h may be NULL)
bool vbs_shape(flacenc_hip_handle* h, uint32_t channels, uint32_t block_size, uint32_t levels, uint64_t total_samples,
               VbsShape* sh) {
  const char* why = nullptr;
  if (channels < 1 || channels > 8) why = "channels not in 1..=8";
  else if (levels < 1 || levels > vbs::MAX_LEVELS) why = "levels not in 1..=5";
  else if (block_size > FLACENC_HIP_MAX_BLOCK_SIZE || block_size % (1u << (levels - 1)) != 0 ||
           (block_size >> (levels - 1)) < vbs::MIN_LEAF)
    why = "block_size must be at most 32767 and divisible by 2^(levels-1), with block_size / 2^(levels-1) >= 256";
  else if (total_samples / block_size >= (1ull << 31) >> (levels - 1))
    why = "too many blocks: the finest level's frame numbers must stay below 2^31";
  if (why) {
    if (h) h->last_error = std::string("encode_variable: ") + why;
    return false;
  }
  sh->n_full = static_cast<uint32_t>(total_samples / block_size);
  sh->tail = static_cast<uint32_t>(total_samples % block_size);
  sh->n_sb = sh->n_full + (sh->tail ? 1u : 0u);
  sh->max_frames = (static_cast<uint64_t>(sh->n_full) << (levels - 1)) + (sh->tail ? 1u : 0u);
  return true;
}

// the packer's slot of one frame (the fixed-blocking bound, 16-byte multiple)
size_t vbs_slot(uint32_t channels, uint32_t block, uint32_t bits_per_sample) {
  return channels == 2 ? flacenc_hip_stereo_frame_bytes_bound(block, bits_per_sample)
                       : flacenc_hip_frame_bytes_bound(channels, block, bits_per_sample);
}
size_t vbs_frame_bound(uint32_t channels, uint32_t block, uint32_t bits_per_sample) {
  return channels == 2 ? flacenc_hip::stereo_frame_bytes_bound(block, bits_per_sample)
                       : flacenc_hip::frame_bytes_bound(channels, block, bits_per_sample);
}
}  // namespace

extern "C" {

size_t flacenc_hip_variable_bytes_bound(uint32_t channels, uint32_t block_size, uint32_t levels,
                                        uint32_t bits_per_sample, uint64_t total_samples) {
  VbsShape sh;
  if (bits_per_sample < 8 || bits_per_sample > 24 || !vbs_shape(nullptr, channels, block_size, levels, total_samples, &sh))
    return 0;
  // the chosen total is at most the sum of the roots; a root is a fixed-blocking frame with one more byte of coded
  // number at most (a sample number of up to 36 bits: 7 bytes, a frame number below 2^31: 6)
  return static_cast<size_t>(sh.n_full) * (vbs_frame_bound(channels, block_size, bits_per_sample) + 1) +
         (sh.tail ? vbs_frame_bound(channels, sh.tail, bits_per_sample) + 1 : 0);
}

size_t flacenc_hip_variable_max_frames(uint32_t block_size, uint32_t levels, uint64_t total_samples) {
  VbsShape sh;
  if (!vbs_shape(nullptr, 1, block_size, levels, total_samples, &sh)) return 0;
  return static_cast<size_t>(sh.max_frames);
}

int flacenc_hip_encode_variable_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                                      uint64_t total_samples, uint32_t channels, uint32_t block_size, uint32_t levels,
                                      size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                      uint64_t first_sample_number, uint8_t* out, size_t out_capacity,
                                      uint64_t* frame_offsets, uint32_t* frame_lengths, uint32_t* frame_block_sizes,
                                      size_t max_frames, uint32_t* split_masks, uint64_t* totals, void* stream) {
  if (!h || !cfg || !totals) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  VbsShape sh;
  if (!vbs_shape(h, channels, block_size, levels, total_samples, &sh)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (first_sample_number > vbs::MAX_SAMPLE_NUMBER || total_samples > vbs::MAX_SAMPLE_NUMBER - first_sample_number) {
    h->last_error = "encode_variable: first_sample_number + total_samples exceeds 2^36";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (!frames || stride < block_size || (out_capacity && !out) ||
      (max_frames && (!frame_offsets || !frame_lengths || !frame_block_sizes))) {
    h->last_error = "encode_variable: null pointer or stride < block_size";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(h, hipSetDevice(h->device));
  if (total_samples == 0) {
    HIP_TRY(h, hipMemsetAsync(totals, 0, 16, s));
    return FLACENC_HIP_OK;
  }
  // scratch plan: per level its packed frames (the packer's strided slots) and lengths
  flacenc_hip::VbsLayout l{};
  l.levels = levels;
  l.superblock = block_size;
  l.n_full = sh.n_full;
  l.tail = sh.tail;
  l.first_sample = first_sample_number;
  size_t pack_bytes = 0, n_lens = 0, frames_bytes = 0, results_bytes = 0;
  const size_t result_bytes = channels == 2 ? sizeof(flacenc_hip_stereo_frame_result)
                                            : channels * sizeof(flacenc_hip_channel_result);
  size_t level_frames[vbs::MAX_LEVELS], level_stride[vbs::MAX_LEVELS];
  for (uint32_t k = 0; k < levels; ++k) {
    const uint32_t b = block_size >> k;
    level_frames[k] = k == 0 ? sh.n_sb : (static_cast<size_t>(sh.n_full) << k);
    level_stride[k] = padded_stride(b);
    l.pack_base[k] = pack_bytes;
    l.pack_stride[k] = vbs_slot(channels, b, bits_per_sample);
    l.len_base[k] = static_cast<uint32_t>(n_lens);
    pack_bytes += a256(level_frames[k] * l.pack_stride[k]);
    n_lens += level_frames[k];
    if (k > 0) frames_bytes = std::max(frames_bytes, level_frames[k] * channels * level_stride[k] * 4);
    results_bytes = std::max(results_bytes, level_frames[k] * result_bytes);
  }
  const size_t slots = static_cast<size_t>(sh.max_frames);
  const size_t o_masks = a256(n_lens * 4), o_counts = o_masks + a256(sh.n_sb * 4), o_first = o_counts + a256(sh.n_sb * 4),
               o_chosen = o_first + a256(sh.n_sb * 8), o_vlen = o_chosen + a256(slots * sizeof(flacenc_hip::VbsChosen)),
               o_voff = o_vlen + a256(slots * 4), o_tot = o_voff + a256(slots * 8), meta_bytes = o_tot + 256;
  int rc;
  if ((rc = ensure(h, h->d_vbs_pack, pack_bytes)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_vbs_results, results_bytes)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_vbs_meta, meta_bytes)) != FLACENC_HIP_OK) return rc;
  if (frames_bytes && (rc = ensure(h, h->d_vbs_frames, frames_bytes)) != FLACENC_HIP_OK) return rc;
  uint8_t* pack = static_cast<uint8_t*>(h->d_vbs_pack.ptr);
  char* meta = static_cast<char*>(h->d_vbs_meta.ptr);
  uint32_t* lens = reinterpret_cast<uint32_t*>(meta);
  l.pack = pack;
  l.lens = lens;
  // every candidate block: the fixed-blocking encode+pack call at its size, frame numbers 0, 1, .. of its level
  auto encode = [&](const int32_t* fr, size_t n, uint32_t b, size_t st, uint32_t first_number, uint8_t* o, size_t o_stride,
                    uint32_t* o_len) -> int {
    if (channels == 2)
      return flacenc_hip_encode_pack_stereo_frames_async(
          h, cfg, fr, n, b, st, bits_per_sample, sample_rate, first_number, 1,
          static_cast<flacenc_hip_stereo_frame_result*>(h->d_vbs_results.ptr), o, o_stride, o_len, stream);
    return flacenc_hip_encode_pack_frames_async(h, cfg, fr, n, channels, b, st, bits_per_sample, sample_rate, first_number,
                                                1, static_cast<flacenc_hip_channel_result*>(h->d_vbs_results.ptr), o,
                                                o_stride, o_len, stream);
  };
  if (sh.n_full && (rc = encode(frames, sh.n_full, block_size, stride, 0, pack, l.pack_stride[0], lens)) != FLACENC_HIP_OK)
    return rc;
  if (sh.tail && (rc = encode(frames + static_cast<size_t>(sh.n_full) * channels * stride, 1, sh.tail, stride, sh.n_full,
                              pack + static_cast<size_t>(sh.n_full) * l.pack_stride[0], l.pack_stride[0],
                              lens + sh.n_full)) != FLACENC_HIP_OK)
    return rc;
  for (uint32_t k = 1; k < levels && sh.n_full; ++k) {
    int32_t* lf = static_cast<int32_t*>(h->d_vbs_frames.ptr);
    HIP_TRY(h, flacenc_hip::launch_reblock(frames, stride, sh.n_full, channels, block_size, k, lf, level_stride[k], s));
    if ((rc = encode(lf, level_frames[k], block_size >> k, level_stride[k], 0, pack + l.pack_base[k], l.pack_stride[k],
                     lens + l.len_base[k])) != FLACENC_HIP_OK)
      return rc;
  }
  // the tree minimum per superblock, each superblock's first output frame, the chosen frames, their byte offsets
  uint32_t* masks = reinterpret_cast<uint32_t*>(meta + o_masks);
  uint32_t* counts = reinterpret_cast<uint32_t*>(meta + o_counts);
  uint64_t* first = reinterpret_cast<uint64_t*>(meta + o_first);
  auto* chosen = reinterpret_cast<flacenc_hip::VbsChosen*>(meta + o_chosen);
  uint32_t* vlen = reinterpret_cast<uint32_t*>(meta + o_vlen);
  uint64_t* voff = reinterpret_cast<uint64_t*>(meta + o_voff);
  uint64_t* tot = reinterpret_cast<uint64_t*>(meta + o_tot);
  HIP_TRY(h, flacenc_hip::launch_vbs_decide(l, masks, counts, s));
  HIP_TRY(h, flacenc_hip::launch_stream_offsets(counts, static_cast<uint32_t>(sh.n_sb), 1, static_cast<uint32_t>(sh.n_sb), 0,
                                                nullptr, first, tot, s));
  HIP_TRY(h, hipMemsetAsync(vlen, 0, slots * 4, s));
  HIP_TRY(h, flacenc_hip::launch_vbs_emit(l, masks, counts, first, static_cast<uint32_t>(slots), chosen, vlen, split_masks, s));
  HIP_TRY(h, flacenc_hip::launch_stream_offsets(vlen, static_cast<uint32_t>(slots), 1, static_cast<uint32_t>(slots), 0,
                                                nullptr, voff, tot + 1, s));
  HIP_TRY(h, flacenc_hip::launch_rehead(l, chosen, voff, tot, tot + 1, static_cast<uint32_t>(slots), out, out_capacity,
                                        frame_offsets, frame_lengths, frame_block_sizes, max_frames, totals, s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_encode_variable(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                                uint64_t total_samples, uint32_t channels, uint32_t block_size, uint32_t levels,
                                size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                uint64_t first_sample_number, uint8_t* out, size_t out_capacity, uint64_t* frame_offsets,
                                uint32_t* frame_lengths, uint32_t* frame_block_sizes, size_t max_frames,
                                uint32_t* split_masks, uint64_t* totals, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE) {
    return drained(h, flacenc_hip_encode_variable_async(h, cfg, frames, total_samples, channels, block_size, levels, stride,
                                                        bits_per_sample, sample_rate, first_sample_number, out,
                                                        out_capacity, frame_offsets, frame_lengths, frame_block_sizes,
                                                        max_frames, split_masks, totals, h->stream), false);
  }
  if (memory_kind != FLACENC_HIP_MEM_HOST || !cfg || !totals) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  VbsShape sh;
  if (!vbs_shape(h, channels, block_size, levels, total_samples, &sh)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (!frames || stride < block_size || (out_capacity && !out) ||
      (max_frames && (!frame_offsets || !frame_lengths || !frame_block_sizes))) {
    h->last_error = "encode_variable: null pointer or stride < block_size";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // host pointers: stage through the handle's device scratch
  const size_t in_bytes = static_cast<size_t>(sh.n_sb) * channels * stride * 4;
  const size_t o_out = a256(in_bytes), o_off = o_out + a256(out_capacity), o_len = o_off + a256(max_frames * 8),
               o_bs = o_len + a256(max_frames * 4), o_masks = o_bs + a256(max_frames * 4),
               o_tot = o_masks + a256(static_cast<size_t>(sh.n_sb) * 4), total = o_tot + 256;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  if ((rc = ensure(h, h->d_vbs_io, total)) != FLACENC_HIP_OK) return rc;
  char* d = static_cast<char*>(h->d_vbs_io.ptr);
  hipStream_t s = h->stream;
  if (in_bytes) HIP_TRY(h, hipMemcpyAsync(d, frames, in_bytes, hipMemcpyHostToDevice, s));
  rc = flacenc_hip_encode_variable_async(h, cfg, reinterpret_cast<const int32_t*>(d), total_samples, channels, block_size,
                                         levels, stride, bits_per_sample, sample_rate, first_sample_number,
                                         reinterpret_cast<uint8_t*>(d + o_out), out_capacity,
                                         reinterpret_cast<uint64_t*>(d + o_off), reinterpret_cast<uint32_t*>(d + o_len),
                                         reinterpret_cast<uint32_t*>(d + o_bs), max_frames,
                                         reinterpret_cast<uint32_t*>(d + o_masks), reinterpret_cast<uint64_t*>(d + o_tot),
                                         s);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(totals, d + o_tot, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (split_masks && sh.n_sb) HIP_TRY(h, hipMemcpyAsync(split_masks, d + o_masks, sh.n_sb * 4, hipMemcpyDeviceToHost, s));
  if (!(totals[0] & FLACENC_HIP_VARIABLE_OVERFLOW) && totals[0]) {
    const size_t n = static_cast<size_t>(totals[0]);
    HIP_TRY(h, hipMemcpyAsync(out, d + o_out, static_cast<size_t>(totals[1]), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(frame_offsets, d + o_off, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(frame_lengths, d + o_len, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(frame_block_sizes, d + o_bs, n * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

}  // extern "C"
