// api_decode.cpp -- the frame decoder's entry points: decode, verify, index (kernels: flac_decode.cpp).
#include "api_internal.h"
#include "flac_decode.h"

using namespace flacenc_hip;

static int check_decode_args(flacenc_hip_handle* h, const uint8_t* bytes, const uint64_t* offsets,
                             const uint32_t* lengths, size_t n_frames, uint32_t channels, uint32_t bits_per_sample,
                             uint32_t max_block_size, const void* rows, size_t stride, const uint32_t* status) {
  if (!bytes || !offsets || !lengths || !rows || !status || channels < 1 || channels > 8 || max_block_size < 1 ||
      max_block_size > 65536 || stride < max_block_size || n_frames > 0x7FFFFFFFull) {
    h->last_error = "decode_frames: null pointer, channels not in 1..=8, max_block_size not in 1..=65536, "
                    "stride < max_block_size or more than 2^31 - 1 frames";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (bits_per_sample < 4 || bits_per_sample > h->max_bps) {
    h->last_error = "decode_frames: bits_per_sample not in 4..=24 (4..=32 with flacenc_hip_set_max_bits_per_sample)";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  return FLACENC_HIP_OK;
}

static int decode_or_verify_async(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                  const uint64_t* offsets, const uint32_t* lengths, size_t n_frames, uint32_t channels,
                                  uint32_t bits_per_sample, uint32_t max_block_size, int32_t* out,
                                  const int32_t* expected, size_t stride, uint32_t* block_sizes, uint64_t* numbers,
                                  uint32_t* status, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  int rc = check_decode_args(h, bytes, offsets, lengths, n_frames, channels, bits_per_sample, max_block_size,
                             out ? static_cast<const void*>(out) : static_cast<const void*>(expected), stride, status);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if ((rc = ensure(h, h->d_dec, flacenc_hip::decode_scratch_bytes(n_frames))) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, flacenc_hip::launch_decode_frames(bytes, n_bytes, offsets, lengths, static_cast<uint32_t>(n_frames),
                                               channels, bits_per_sample, max_block_size, h->max_bps, out, expected,
                                               stride, block_sizes, numbers, status, h->d_dec.ptr,
                                               static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

extern "C" {

int flacenc_hip_decode_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, size_t n_frames, uint32_t channels,
                                    uint32_t bits_per_sample, uint32_t max_block_size, int32_t* out, size_t stride,
                                    uint32_t* block_sizes, uint64_t* numbers, uint32_t* status, void* stream) {
  if (h && n_frames && !block_sizes) {
    h->last_error = "decode_frames: block_sizes is NULL";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return decode_or_verify_async(h, bytes, UINT64_MAX, offsets, lengths, n_frames, channels, bits_per_sample,
                                max_block_size, out, nullptr, stride, block_sizes, numbers, status, stream);
}

int flacenc_hip_verify_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, size_t n_frames, uint32_t channels,
                                    uint32_t bits_per_sample, uint32_t max_block_size, const int32_t* expected,
                                    size_t stride, uint32_t* status, void* stream) {
  return decode_or_verify_async(h, bytes, UINT64_MAX, offsets, lengths, n_frames, channels, bits_per_sample,
                                max_block_size, nullptr, expected, stride, nullptr, nullptr, status, stream);
}

int flacenc_hip_decode_frames(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                              const uint32_t* lengths, size_t n_frames, uint32_t channels, uint32_t bits_per_sample,
                              uint32_t max_block_size, int32_t* out, size_t stride, uint32_t* block_sizes,
                              uint64_t* numbers, uint32_t* status, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE) {
    if (n_frames && !block_sizes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    return drained(h, decode_or_verify_async(h, bytes, n_bytes, offsets, lengths, n_frames, channels, bits_per_sample,
                                             max_block_size, out, nullptr, stride, block_sizes, numbers, status, h->stream),
                   n_frames == 0);
  }
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  int rc = check_decode_args(h, bytes, offsets, lengths, n_frames, channels, bits_per_sample, max_block_size, out,
                             stride, status);
  if (rc != FLACENC_HIP_OK) return rc;
  if (!block_sizes) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  // host pointers: stage through the handle's device scratch
  const size_t dstride = padded_stride(max_block_size);
  const size_t o_off = a256(n_bytes), o_len = o_off + a256(n_frames * 8), o_out = o_len + a256(n_frames * 4),
               o_bs = o_out + a256(n_frames * channels * dstride * 4), o_num = o_bs + a256(n_frames * 4),
               o_st = o_num + a256(n_frames * 8), total = o_st + a256(n_frames * 4);
  HIP_TRY(h, hipSetDevice(h->device));
  if ((rc = ensure(h, h->d_dec_io, total)) != FLACENC_HIP_OK) return rc;
  char* d = static_cast<char*>(h->d_dec_io.ptr);
  hipStream_t s = h->stream;
  HIP_TRY(h, hipMemcpyAsync(d, bytes, n_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d + o_off, offsets, n_frames * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d + o_len, lengths, n_frames * 4, hipMemcpyHostToDevice, s));
  rc = decode_or_verify_async(h, reinterpret_cast<const uint8_t*>(d), n_bytes,
                              reinterpret_cast<const uint64_t*>(d + o_off), reinterpret_cast<const uint32_t*>(d + o_len),
                              n_frames, channels, bits_per_sample, max_block_size, reinterpret_cast<int32_t*>(d + o_out),
                              nullptr, dstride, reinterpret_cast<uint32_t*>(d + o_bs),
                              reinterpret_cast<uint64_t*>(d + o_num), reinterpret_cast<uint32_t*>(d + o_st), s);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpy2DAsync(out, stride * 4, d + o_out, dstride * 4, static_cast<size_t>(max_block_size) * 4,
                              n_frames * channels, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(block_sizes, d + o_bs, n_frames * 4, hipMemcpyDeviceToHost, s));
  if (numbers) HIP_TRY(h, hipMemcpyAsync(numbers, d + o_num, n_frames * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(status, d + o_st, n_frames * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_index_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, uint32_t channels,
                                   uint32_t bits_per_sample, size_t max_frames, uint64_t* offsets, uint32_t* lengths,
                                   uint64_t* n_frames, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (!n_frames || (n_bytes && !bytes) || (max_frames && (!offsets || !lengths)) || channels < 1 || channels > 8 ||
      max_frames > 0x3FFFFFFFull || n_bytes > (static_cast<uint64_t>(0xFFFFFFFFu) << 12)) {
    h->last_error = "index_frames: null pointer, channels not in 1..=8, max_frames >= 2^30 or n_bytes >= 16 TiB";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (bits_per_sample < 4 || bits_per_sample > h->max_bps) {
    h->last_error = "index_frames: bits_per_sample not in 4..=24 (4..=32 with flacenc_hip_set_max_bits_per_sample)";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t cap = flacenc_hip::index_candidate_capacity(max_frames);
  int rc = ensure(h, h->d_idx, flacenc_hip::index_scratch_bytes(n_bytes, cap));
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, flacenc_hip::launch_index_frames(bytes, n_bytes, channels, bits_per_sample, h->max_bps, max_frames, offsets,
                                              lengths,
                                              n_frames, h->d_idx.ptr, cap, static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

}  // extern "C"
