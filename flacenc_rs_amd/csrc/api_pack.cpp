// api_pack.cpp -- Frame::write for batches, frame lengths, the wire format of the exchange, stream offsets and placement
// (kernels: frame_pack.cpp).
#include "api_internal.h"

namespace flacenc_hip {

// y = x^(8 per) mod P and its powers for the CRC-16 slice combination (see frame_pack.h)
void fill_crc_powers(uint32_t lds_words, uint32_t* crc_per, uint16_t crc_pow[32]) {
  auto mulmod = [](uint32_t x, uint32_t y) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
      r <<= 1;
      if (r & 0x10000u) r ^= 0x18005u;
      if ((y >> i) & 1u) r ^= x;
    }
    return r & 0xFFFFu;
  };
  *crc_per = (lds_words * 4 + 255) / 256;
  uint32_t y = 1;
  for (uint32_t i = 0; i < 8 * *crc_per; ++i) y = mulmod(y, 2);  // times x
  uint32_t acc = 1;
  for (int i = 0; i < 16; ++i) {
    crc_pow[i] = static_cast<uint16_t>(acc);
    acc = mulmod(acc, y);
  }
  const uint32_t y16 = acc;  // y^16
  acc = 1;
  for (int i = 0; i < 16; ++i) {
    crc_pow[16 + i] = static_cast<uint16_t>(acc);
    acc = mulmod(acc, y16);
  }
}

// FrameHeader's constant part for a launch (bitrepr.rs:373-419 as encode_frame_impl fills it,
// coding.rs:431-436): spec tags and the extra bytes that follow the frame number
void fill_header_specs(flacenc_hip::FramePackArgs& a, uint32_t block_size, uint32_t sample_rate,
                       uint32_t bits_per_sample) {
  // BlockSizeSpec::from_size / tag / extra bits, datatype.rs:1239-1294
  uint32_t bs_tag = 0, extra_len = 0;
  a.extra[0] = a.extra[1] = a.extra[2] = a.extra[3] = 0;
  if (block_size == 192) bs_tag = 1;
  for (uint32_t x = 0; x < 4 && !bs_tag; ++x)
    if (block_size == (576u << x)) bs_tag = 2 + x;
  for (uint32_t x = 0; x < 8 && !bs_tag; ++x)
    if (block_size == (256u << x)) bs_tag = 8 + x;
  if (!bs_tag) {
    if (block_size <= 256) {
      bs_tag = 6;
      a.extra[extra_len++] = static_cast<uint8_t>(block_size - 1);
    } else {
      bs_tag = 7;
      a.extra[extra_len++] = static_cast<uint8_t>((block_size - 1) >> 8);
      a.extra[extra_len++] = static_cast<uint8_t>(block_size - 1);
    }
  }
  // SampleRateSpec::from_freq / tag / extra bits, datatype.rs:1427-1453, 1503-1543 (Unspecified if
  // not representable, coding.rs:434-435)
  static const uint32_t known[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  uint32_t sr_tag = 0;
  for (uint32_t t = 1; t < 12; ++t)
    if (sample_rate == known[t]) sr_tag = t;
  if (!sr_tag && sample_rate) {
    if (sample_rate % 1000 == 0 && sample_rate / 1000 <= 255) {
      sr_tag = 12;
      a.extra[extra_len++] = static_cast<uint8_t>(sample_rate / 1000);
    } else if (sample_rate % 10 == 0 && sample_rate / 10 <= 65535) {
      sr_tag = 14;
      a.extra[extra_len++] = static_cast<uint8_t>((sample_rate / 10) >> 8);
      a.extra[extra_len++] = static_cast<uint8_t>(sample_rate / 10);
    } else if (sample_rate <= 65535) {
      sr_tag = 13;
      a.extra[extra_len++] = static_cast<uint8_t>(sample_rate >> 8);
      a.extra[extra_len++] = static_cast<uint8_t>(sample_rate);
    }
  }
  // SampleSizeSpec::from_bits, datatype.rs:1350-1360
  uint32_t ss_tag = 0;
  switch (bits_per_sample) {
    case 8: ss_tag = 1; break;
    case 12: ss_tag = 2; break;
    case 16: ss_tag = 4; break;
    case 20: ss_tag = 5; break;
    case 24: ss_tag = 6; break;
    default: ss_tag = 0; break;
  }
  a.header_mid = (bs_tag << 12) | (sr_tag << 8) | (ss_tag << 1);
  a.extra_len = extra_len;
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" {

size_t flacenc_hip_frame_bytes_bound(uint32_t channels, uint32_t block_size, uint32_t bits_per_sample) {
  return (flacenc_hip::frame_bytes_bound(channels, block_size, bits_per_sample) + 15) & ~static_cast<size_t>(15);
}

size_t flacenc_hip_stereo_frame_bytes_bound(uint32_t block_size, uint32_t bits_per_sample) {
  return (flacenc_hip::stereo_frame_bytes_bound(block_size, bits_per_sample) + 15) & ~static_cast<size_t>(15);
}

// Frame::write for a batch: `results` (2-channel records) or `chan_results` + channels
static int enqueue_pack(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                        uint32_t block_size, size_t stride, const flacenc_hip_stereo_frame_result* results,
                        const flacenc_hip_channel_result* chan_results, const int32_t* residual,
                        size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                        uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                        size_t out_stride, uint32_t* out_len, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  const size_t bound = chan_results ? flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample)
                                    : flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample);
  if (chan_results && (channels < 1 || channels > 8)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (!frames || (!results && !chan_results) || !residual || !out || !out_len || stride < block_size || residual_stride < block_size ||
      block_size < 1 || block_size > FLACENC_HIP_MAX_BLOCK_SIZE ||
      bits_per_sample < 8 || bits_per_sample > 24 || n_frames > 0x7FFFFFFFull ||
      (reinterpret_cast<uintptr_t>(out) & 15) || (out_stride & 15) ||
      out_stride < bound) {
    h->last_error = "pack_stereo_frames: null pointer, bad size, or out_stride below flacenc_hip_stereo_frame_bytes_bound";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // frame numbers must stay below 2^31 (encode_fixed_size_frame, coding.rs:587-591)
  const unsigned long long last = static_cast<unsigned long long>(first_frame_number) +
                                  static_cast<unsigned long long>(n_frames - 1) * frame_number_step;
  if (last >= (1ull << 31)) {
    h->last_error = "pack_stereo_frames: frame_number must be below 2^31";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  flacenc_hip::FramePackArgs a;
  a.frames = frames;
  a.stride = stride;
  a.block_size = block_size;
  a.n_frames = static_cast<uint32_t>(n_frames);
  a.results = results;
  a.chan_results = chan_results;
  a.channels = chan_results ? channels : 2u;
  a.residual = residual;
  a.residual_stride = residual_stride;
  a.bits_per_sample = bits_per_sample;
  a.first_frame_number = first_frame_number;
  a.frame_number_step = frame_number_step;
  a.out = out;
  a.out_stride = out_stride;
  a.out_len = out_len;
  fill_header_specs(a, block_size, sample_rate, bits_per_sample);
  a.lds_words = static_cast<uint32_t>(bound / 4 + 4);
  fill_crc_powers(a.lds_words, &a.crc_per, a.crc_pow);
  if (static_cast<size_t>(a.lds_words) * 4 > 150 * 1024) {
    h->last_error = "pack_stereo_frames: frame too large for the LDS bit buffer (block_size x bits_per_sample)";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  // the list of frames with escaped partitions between the packer's two launches (FramePackArgs::escape_list); its
  // counters are zero whenever no pack is in flight, a new buffer's are cleared here
  {
    const size_t before = h->d_esc.cap;
    int rc = flacenc_hip::ensure(h, h->d_esc, (16 + n_frames) * sizeof(uint32_t));
    if (rc != FLACENC_HIP_OK) return rc;
    if (h->d_esc.cap != before) HIP_TRY(h, hipMemsetAsync(h->d_esc.ptr, 0, 64, static_cast<hipStream_t>(stream)));
    a.escape_list = static_cast<uint32_t*>(h->d_esc.ptr);
  }
  HIP_TRY(h, flacenc_hip::launch_frame_pack(a, static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

// The blocking packers on host pointers (arguments checked by the caller, exactly one of `results` / `chan_results`
// given): rows, records and packed frames staged through the handle's scratch around enqueue_pack.
static int pack_host_frames(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                            uint32_t block_size, size_t stride, const flacenc_hip_stereo_frame_result* results,
                            const flacenc_hip_channel_result* chan_results, const int32_t* residual,
                            size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                            uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out, size_t out_stride,
                            uint32_t* out_len) {
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  const size_t n_rows = n_frames * channels;
  const size_t record_bytes = results ? n_frames * sizeof(*results) : n_rows * sizeof(*chan_results);
  const size_t dstride = padded_stride(block_size);
  const size_t ostride = results ? flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample)
                                 : flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample);
  if (out_stride < ostride) {
    h->last_error = results ? "pack_stereo_frames: out_stride below flacenc_hip_stereo_frame_bytes_bound"
                            : "pack_frames: out_stride below flacenc_hip_frame_bytes_bound";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if ((rc = ensure(h, h->d_samples, n_rows * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_rows * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_results, record_bytes)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_out, n_frames * ostride)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_outlen, n_frames * 4)) != FLACENC_HIP_OK) return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, frames, stride, block_size, n_rows)) != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_device(h, h->d_residual, residual, residual_stride, block_size, n_rows)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->d_results.ptr, results ? static_cast<const void*>(results) : chan_results, record_bytes,
                            hipMemcpyHostToDevice, s));
  rc = enqueue_pack(h, static_cast<const int32_t*>(h->d_samples.ptr), n_frames, channels, block_size, dstride,
                    results ? static_cast<const flacenc_hip_stereo_frame_result*>(h->d_results.ptr) : nullptr,
                    results ? nullptr : static_cast<const flacenc_hip_channel_result*>(h->d_results.ptr),
                    static_cast<const int32_t*>(h->d_residual.ptr), dstride, bits_per_sample, sample_rate,
                    first_frame_number, frame_number_step, static_cast<uint8_t*>(h->d_out.ptr), ostride,
                    static_cast<uint32_t*>(h->d_outlen.ptr), s);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpy2DAsync(out, out_stride, h->d_out.ptr, ostride, ostride, n_frames, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(out_len, h->d_outlen.ptr, n_frames * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_pack_stereo_frames_async(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames,
                                         uint32_t block_size, size_t stride,
                                         const flacenc_hip_stereo_frame_result* results, const int32_t* residual,
                                         size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                         uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                                         size_t out_stride, uint32_t* out_len, void* stream) {
  if (!results && n_frames) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return enqueue_pack(h, frames, n_frames, 2, block_size, stride, results, nullptr, residual, residual_stride,
                      bits_per_sample, sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len,
                      stream);
}

int flacenc_hip_pack_frames_async(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                                  uint32_t block_size, size_t stride, const flacenc_hip_channel_result* results,
                                  const int32_t* residual, size_t residual_stride, uint32_t bits_per_sample,
                                  uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                                  uint8_t* out, size_t out_stride, uint32_t* out_len, void* stream) {
  if (!results && n_frames) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return enqueue_pack(h, frames, n_frames, channels, block_size, stride, nullptr, results, residual, residual_stride,
                      bits_per_sample, sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len,
                      stream);
}

int flacenc_hip_stereo_frame_lengths_async(flacenc_hip_handle* h, const flacenc_hip_stereo_frame_result* results,
                                           size_t n_frames, uint32_t block_size, uint32_t bits_per_sample,
                                           uint32_t sample_rate, uint32_t first_frame_number,
                                           uint32_t frame_number_step, uint32_t* out_len, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!results || !out_len || n_frames > 0x7FFFFFFFull) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const unsigned long long last = static_cast<unsigned long long>(first_frame_number) +
                                  static_cast<unsigned long long>(n_frames - 1) * frame_number_step;
  if (last >= (1ull << 31)) {
    h->last_error = "stereo_frame_lengths: frame_number must be below 2^31";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  flacenc_hip::FramePackArgs a{};
  a.results = results;
  a.n_frames = static_cast<uint32_t>(n_frames);
  a.first_frame_number = first_frame_number;
  a.frame_number_step = frame_number_step;
  a.out_len = out_len;
  fill_header_specs(a, block_size, sample_rate, bits_per_sample);
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, flacenc_hip::launch_frame_lengths(a, static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

// 2^finest_partition_order of a block (src/rice.rs:157-165 with a warm-up of at most 64 samples: the bound over all
// predictor orders): how many of a subframe record's rice_params can be non-zero
static uint32_t finest_partitions(uint32_t block_size) {
  uint32_t order = 0, n = block_size;
  while (order < 8 && n % 2 == 0 && n / 2 >= 64) {
    n /= 2;
    ++order;
  }
  return 1u << order;
}

size_t flacenc_hip_frame_wire_bytes(uint32_t block_size) { return 48 + 2 * (96 + static_cast<size_t>(finest_partitions(block_size))); }

int flacenc_hip_stereo_frame_wire_async(flacenc_hip_handle* h, const flacenc_hip_stereo_frame_result* results,
                                        size_t n_frames, uint32_t block_size, uint32_t bits_per_sample,
                                        uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                                        uint8_t* wire, size_t wire_stride, uint32_t* out_len, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!results || !wire || n_frames > 0x7FFFFFFFull || wire_stride < flacenc_hip_frame_wire_bytes(block_size))
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const unsigned long long last = static_cast<unsigned long long>(first_frame_number) +
                                  static_cast<unsigned long long>(n_frames - 1) * frame_number_step;
  if (last >= (1ull << 31)) {
    h->last_error = "stereo_frame_wire: frame_number must be below 2^31";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  flacenc_hip::FramePackArgs a{};
  a.results = results;
  a.n_frames = static_cast<uint32_t>(n_frames);
  a.first_frame_number = first_frame_number;
  a.frame_number_step = frame_number_step;
  a.out_len = out_len;
  fill_header_specs(a, block_size, sample_rate, bits_per_sample);
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, flacenc_hip::launch_frame_wire(a, finest_partitions(block_size), wire, wire_stride,
                                            static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

int flacenc_hip_stream_offsets_async(flacenc_hip_handle* h, const uint32_t* gathered_lengths, size_t n_frames_total,
                                     uint32_t world, uint64_t header_bytes, uint32_t* lengths_stream,
                                     uint64_t* offsets, uint64_t* total, void* stream) {
  if (!h || world == 0 || !total || n_frames_total > 0x7FFFFFFFull) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames_total && (!gathered_lengths || !offsets)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const uint32_t n = static_cast<uint32_t>(n_frames_total);
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, flacenc_hip::launch_stream_offsets(gathered_lengths, n, world, (n + world - 1) / world, header_bytes,
                                                lengths_stream, offsets, total, static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

int flacenc_hip_place_frames_async(flacenc_hip_handle* h, const uint8_t* src, const uint64_t* src_offsets,
                                   const uint32_t* lengths, size_t n_frames, uint8_t* dst,
                                   const uint64_t* dst_offsets, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!src || !src_offsets || !lengths || !dst || !dst_offsets || n_frames > 0x7FFFFFFFull)
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, flacenc_hip::launch_place_frames(src, src_offsets, lengths, dst, dst_offsets,
                                              static_cast<uint32_t>(n_frames), static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

int flacenc_hip_pack_stereo_frames(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames,
                                   uint32_t block_size, size_t stride,
                                   const flacenc_hip_stereo_frame_result* results, const int32_t* residual,
                                   size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                   uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                                   size_t out_stride, uint32_t* out_len, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, flacenc_hip_pack_stereo_frames_async(h, frames, n_frames, block_size, stride, results, residual,
                                                           residual_stride, bits_per_sample, sample_rate, first_frame_number,
                                                           frame_number_step, out, out_stride, out_len, h->stream),
                   n_frames == 0);
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!frames || !results || !residual || !out || !out_len || stride < block_size || residual_stride < block_size)
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return pack_host_frames(h, frames, n_frames, 2, block_size, stride, results, nullptr, residual, residual_stride,
                          bits_per_sample, sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len);
}

int flacenc_hip_pack_frames(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                            uint32_t block_size, size_t stride, const flacenc_hip_channel_result* results,
                            const int32_t* residual, size_t residual_stride, uint32_t bits_per_sample,
                            uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                            uint8_t* out, size_t out_stride, uint32_t* out_len, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, flacenc_hip_pack_frames_async(h, frames, n_frames, channels, block_size, stride, results, residual,
                                                    residual_stride, bits_per_sample, sample_rate, first_frame_number,
                                                    frame_number_step, out, out_stride, out_len, h->stream),
                   n_frames == 0);
  if (memory_kind != FLACENC_HIP_MEM_HOST || channels < 1 || channels > 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!frames || !results || !residual || !out || !out_len || stride < block_size || residual_stride < block_size)
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return pack_host_frames(h, frames, n_frames, channels, block_size, stride, nullptr, results, residual, residual_stride,
                          bits_per_sample, sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len);
}

}  // extern "C"
