// api_stream.cpp -- the streaming host path: packed PCM in caller memory to FLAC frames in caller memory, chunked over
// two slots of pinned staging and three streams.
#include "api_internal.h"

using namespace flacenc_hip;

namespace flacenc_hip {
bool is_pinned(const void* p) {
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // plain malloc memory: not an error for the caller
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

int ensure_pinned(flacenc_hip_handle* h, void** slot, size_t* cap_field, size_t bytes) {
  if (bytes <= *cap_field && slot[0] && slot[1]) return FLACENC_HIP_OK;
  for (int i = 0; i < 2; ++i) {
    if (slot[i]) HIP_TRY(h, hipHostFree(slot[i]));
    slot[i] = nullptr;
  }
  *cap_field = 0;
  const size_t want = bytes + bytes / 8 + 4096;
  for (int i = 0; i < 2; ++i) HIP_TRY(h, hipHostMalloc(&slot[i], want, hipHostMallocDefault));
  *cap_field = want;
  return FLACENC_HIP_OK;
}

int ensure_stream_objects(flacenc_hip_handle* h) {
  if (h->s_in) return FLACENC_HIP_OK;
  HIP_TRY(h, hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
  HIP_TRY(h, hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_h2d[i], hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fill[i], hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_pack[i], hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_d2h[i], hipEventDisableTiming));
  }
  return FLACENC_HIP_OK;
}

// staging copies for pageable caller memory run on the caller's thread + the handle's helper threads
int ensure_copy_pool(flacenc_hip_handle* h, const char* what) {
  if (h->copy_pool) return FLACENC_HIP_OK;
  const int want = h->host_threads < 0 ? 4 : h->host_threads;  // total, the caller's thread included
  // (thread creation can throw std::system_error, vector growth std::bad_alloc: nothing unwinds across the ABI)
  try {
    h->copy_pool.reset(new CopyPool(want > 1 ? static_cast<unsigned>(want - 1) : 0u));
  } catch (...) {
    h->copy_pool.reset();
  }
  if (!h->copy_pool) {
    try {
      h->copy_pool.reset(new CopyPool(0u));  // no helper threads: plain memcpy on the caller's thread
    } catch (...) {
      h->last_error = std::string(what) + ": out of host memory";
      return FLACENC_HIP_ERR_DEVICE;
    }
  }
  return FLACENC_HIP_OK;
}
}  // namespace flacenc_hip

extern "C" {

int flacenc_hip_fill_le_bytes_async(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples,
                                    uint32_t channels, uint32_t bytes_per_sample, size_t n_frames,
                                    uint32_t block_size, int32_t* frames, size_t stride, void* stream) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!bytes || !frames || channels < 1 || channels > 8 || bytes_per_sample < 1 || bytes_per_sample > 4 ||
      block_size < 1 || block_size > FLACENC_HIP_MAX_BLOCK_SIZE || stride < block_size || n_frames > 0xFFFFull) {
    h->last_error = "fill_le_bytes: null pointer, channels not in 1..=8, bytes_per_sample not in 1..=4, or > 65535 frames";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, flacenc_hip::launch_fill_le_bytes(bytes, channels, bytes_per_sample, total_samples,
                                               static_cast<uint32_t>(n_frames), block_size, frames, stride,
                                               static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

int flacenc_hip_fill_le_bytes(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples,
                              uint32_t channels, uint32_t bytes_per_sample, size_t n_frames, uint32_t block_size,
                              int32_t* frames, size_t stride, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE) {
    return drained(h, flacenc_hip_fill_le_bytes_async(h, bytes, total_samples, channels, bytes_per_sample, n_frames,
                                                      block_size, frames, stride, h->stream), n_frames == 0);
  }
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!bytes || !frames || channels < 1 || channels > 8 || bytes_per_sample < 1 || bytes_per_sample > 4 ||
      stride < block_size)
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  const uint64_t wanted = static_cast<uint64_t>(n_frames) * block_size;
  const uint64_t have = total_samples < wanted ? total_samples : wanted;
  const size_t nbytes = static_cast<size_t>(have) * channels * bytes_per_sample;
  const size_t dstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_out, nbytes + 16)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_samples, n_frames * channels * dstride * 4)) != FLACENC_HIP_OK) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(h, hipMemcpyAsync(h->d_out.ptr, bytes, nbytes, hipMemcpyHostToDevice, s));
  rc = flacenc_hip_fill_le_bytes_async(h, static_cast<const uint8_t*>(h->d_out.ptr), have, channels, bytes_per_sample,
                                       n_frames, block_size, static_cast<int32_t*>(h->d_samples.ptr), dstride, s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, frames, stride, h->d_samples, block_size, n_frames * channels)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_encode_pcm_stereo(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                                  uint64_t total_samples, uint32_t bytes_per_sample, uint32_t bits_per_sample,
                                  uint32_t block_size, uint32_t sample_rate, uint32_t first_frame_number,
                                  uint32_t frame_number_step, uint8_t* out, size_t out_capacity, uint32_t* out_len,
                                  uint64_t* out_total) {
  return flacenc_hip_encode_pcm(h, cfg, pcm, total_samples, 2, bytes_per_sample, bits_per_sample, block_size,
                                sample_rate, first_frame_number, frame_number_step, out, out_capacity, out_len, out_total);
}

int flacenc_hip_encode_pcm(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                           uint64_t total_samples, uint32_t channels, uint32_t bytes_per_sample,
                           uint32_t bits_per_sample, uint32_t block_size, uint32_t sample_rate,
                           uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out, size_t out_capacity,
                           uint32_t* out_len, uint64_t* out_total) {
  if (!h || !cfg || !out_total) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  *out_total = 0;
  h->last_stream_chunk = h->last_stream_chunks = 0;  // flacenc_hip_debug_last_stream_plan: no chunk has run yet
  if (total_samples == 0) return FLACENC_HIP_OK;
  if (!pcm || !out || !out_len || channels < 1 || channels > 8 || bytes_per_sample < 1 || bytes_per_sample > 4 ||
      block_size < FLACENC_HIP_MIN_BLOCK_SIZE || block_size > FLACENC_HIP_MAX_BLOCK_SIZE) {
    h->last_error = "encode_pcm: null pointer, channels not in 1..=8, bytes_per_sample not in 1..=4 or block_size "
                    "not in 64..=32767";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // more than 24 bits: the wide step, after flacenc_hip_set_max_encode_bits_per_sample(h, 32) and in 4-byte samples
  // (without the opt-in the frame-level calls below refuse the depth as they always have)
  const bool wide = is_wide(bits_per_sample) && bits_per_sample <= h->max_encode_bps;
  if (wide && bytes_per_sample != 4) {
    h->last_error = "encode_pcm: more than 24 bits per sample come in 4-byte samples";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const bool stereo = channels == 2;
  const uint64_t n_full = total_samples / block_size;
  const uint32_t tail = static_cast<uint32_t>(total_samples % block_size);
  // (a last block shorter than MIN_BLOCK_SIZE_FOR_PREDICTION is a frame like any other: encode_subframe skips
  // its predictors, coding.rs:396, and the frame-level calls below do the same)
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  if ((rc = ensure_stream_objects(h)) != FLACENC_HIP_OK) return rc;
  // chunks of whole frames: big enough to run the kernels at full occupancy (>= 768 workgroups),
  // small enough that two slots of staging stay modest and the pipeline has several stages in flight
  const size_t frame_in_bytes = static_cast<size_t>(block_size) * channels * bytes_per_sample;
  size_t chunk = (48u << 20) / frame_in_bytes;
  chunk = chunk < 768 ? 768 : (chunk > 8192 ? 8192 : chunk);
  // (test hook flacenc_hip_debug_set_stream_chunk, hooks library only: seams after a handful of frames)
  if (h->stream_chunk_override) chunk = h->stream_chunk_override;
  // never more than the call has: staging, device buffers and the candidates' scratch are all sized from it
  // (a one-frame call of 8 channels x 32767 samples would otherwise pin gigabytes)
  if (chunk > n_full) chunk = n_full ? static_cast<size_t>(n_full) : 1;
  const size_t bound = stereo ? flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample)
                              : flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample);
  const size_t ostride = (bound + 15) & ~static_cast<size_t>(15);
  const bool in_pinned = is_pinned(pcm), out_pinned = is_pinned(out);
  h->last_stream_in_pinned = in_pinned;  // flacenc_hip_debug_last_stream_buffers
  h->last_stream_out_pinned = out_pinned;
  const size_t dstride = padded_stride(block_size);
  if (!in_pinned && (rc = ensure_pinned(h, h->pin_in, &h->pin_in_cap, chunk * frame_in_bytes)) != FLACENC_HIP_OK) return rc;
  if (!out_pinned && (rc = ensure_pinned(h, h->pin_out, &h->pin_out_cap, chunk * ostride)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure_pinned(h, h->pin_meta, &h->pin_meta_cap, chunk * 4 + 16)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_samples, chunk * channels * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_results, chunk * (stereo ? sizeof(flacenc_hip_stereo_frame_result)
                                                     : channels * sizeof(flacenc_hip_channel_result)))) != FLACENC_HIP_OK)
    return rc;
  if (wide && (rc = ensure(h, h->d_wide, chunk * wideenc::roles_of(channels) * sizeof(wideenc::SubRecord))) != FLACENC_HIP_OK)
    return rc;
  for (int i = 0; i < 2; ++i) {
    if ((rc = ensure(h, h->d_pcm[i], chunk * frame_in_bytes + 16)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_pack[i], chunk * ostride)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_plen[i], chunk * 4 + 16)) != FLACENC_HIP_OK) return rc;   // lengths, then the total
    if ((rc = ensure(h, h->d_poff[i], chunk * 16 + 16)) != FLACENC_HIP_OK) return rc;  // src + dst offsets
    if ((rc = ensure(h, h->d_cont[i], chunk * ostride)) != FLACENC_HIP_OK) return rc;
  }

  struct Chunk {
    uint64_t first_frame;  // index within this call
    size_t frames;
    uint32_t n;            // block size of its frames
  };
  std::vector<Chunk> chunks;
  for (uint64_t f = 0; f < n_full; f += chunk)
    chunks.push_back({f, static_cast<size_t>(n_full - f < chunk ? n_full - f : chunk), block_size});
  if (tail) chunks.push_back({n_full, 1, tail});
  h->last_stream_chunk = chunk;
  h->last_stream_chunks = chunks.size();

  if ((!in_pinned || !out_pinned) && (rc = ensure_copy_pool(h, "encode_pcm")) != FLACENC_HIP_OK) return rc;
  uint64_t written = 0;
  // A chunk's way out has two steps so that the host never idles on a transfer: start_out waits for the
  // chunk's lengths and starts the device -> host copy of exactly its bytes (contiguous on the device
  // already); finish_out -- one chunk later, after the next chunk's staging copy in -- waits for that
  // transfer and hands the bytes to the caller.
  struct Pending {
    uint64_t at = 0, bytes = 0;
  } pending[2];
  auto start_out = [&](size_t ci) -> int {
    const Chunk& c = chunks[ci];
    const int s = static_cast<int>(ci & 1);
    HIP_TRY(h, hipEventSynchronize(h->ev_pack[s]));  // lengths + total are in pin_meta[s]
    const uint32_t* lens = static_cast<const uint32_t*>(h->pin_meta[s]);
    uint64_t bytes = 0;
    for (size_t f = 0; f < c.frames; ++f) bytes += lens[f];
    if (written + bytes > out_capacity) {
      h->last_error = "encode_pcm: out_capacity too small";
      return FLACENC_HIP_ERR_BAD_ARGUMENT;
    }
    std::memcpy(out_len + c.first_frame, lens, c.frames * 4);
    HIP_TRY(h, hipMemcpyAsync(out_pinned ? static_cast<void*>(out + written) : h->pin_out[s], h->d_cont[s].ptr, bytes,
                              hipMemcpyDeviceToHost, h->s_out));
    HIP_TRY(h, hipEventRecord(h->ev_d2h[s], h->s_out));
    pending[s].at = written;
    pending[s].bytes = bytes;
    written += bytes;
    return FLACENC_HIP_OK;
  };
  auto finish_out = [&](size_t ci) -> int {
    if (out_pinned) return FLACENC_HIP_OK;
    const int s = static_cast<int>(ci & 1);
    HIP_TRY(h, hipEventSynchronize(h->ev_d2h[s]));
    h->copy_pool->copy(out + pending[s].at, h->pin_out[s], pending[s].bytes);
    return FLACENC_HIP_OK;
  };

  // an error half way leaves work in flight on three streams: drain them before handing the handle back
  struct Drain {
    flacenc_hip_handle* h;
    bool armed = true;
    ~Drain() {
      if (!armed) return;
      (void)hipStreamSynchronize(h->s_in);
      (void)hipStreamSynchronize(h->stream);
      (void)hipStreamSynchronize(h->s_out);
    }
  } drain_on_error{h};
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const Chunk& c = chunks[ci];
    const int s = static_cast<int>(ci & 1);
    const size_t in_bytes = c.frames * static_cast<size_t>(c.n) * channels * bytes_per_sample;
    const uint8_t* src = pcm + c.first_frame * frame_in_bytes;
    // 1. host -> device: packed PCM (2..3 bytes per sample instead of 4)
    if (ci >= 2) HIP_TRY(h, hipStreamWaitEvent(h->s_in, h->ev_fill[s], 0));  // d_pcm[s] has been consumed
    if (in_pinned) {
      HIP_TRY(h, hipMemcpyAsync(h->d_pcm[s].ptr, src, in_bytes, hipMemcpyHostToDevice, h->s_in));
    } else {
      if (ci >= 2) HIP_TRY(h, hipEventSynchronize(h->ev_h2d[s]));  // pin_in[s] has been sent
      h->copy_pool->copy(h->pin_in[s], src, in_bytes);
      HIP_TRY(h, hipMemcpyAsync(h->d_pcm[s].ptr, h->pin_in[s], in_bytes, hipMemcpyHostToDevice, h->s_in));
    }
    HIP_TRY(h, hipEventRecord(h->ev_h2d[s], h->s_in));
    // 2. compute stream: widen + de-interleave, analyse + decide + Frame::write, compact
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_h2d[s], 0));
    const size_t cstride = padded_stride(c.n);
    rc = flacenc_hip_fill_le_bytes_async(h, static_cast<const uint8_t*>(h->d_pcm[s].ptr),
                                         static_cast<uint64_t>(c.frames) * c.n, channels, bytes_per_sample, c.frames, c.n,
                                         static_cast<int32_t*>(h->d_samples.ptr), cstride, h->stream);
    if (rc != FLACENC_HIP_OK) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_fill[s], h->stream));
    if (ci >= 2) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_d2h[s], 0));  // d_cont[s] has been copied out
    const size_t cbound = ((stereo ? flacenc_hip_stereo_frame_bytes_bound(c.n, bits_per_sample)
                                   : flacenc_hip_frame_bytes_bound(channels, c.n, bits_per_sample)) + 15) & ~static_cast<size_t>(15);
    uint32_t* dlen = static_cast<uint32_t*>(h->d_plen[s].ptr);
    const uint32_t number = first_frame_number + static_cast<uint32_t>(c.first_frame) * frame_number_step;
    if (wide) {
      rc = encode_pack_frames_wide(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), c.frames, channels,
                                                     c.n, cstride, bits_per_sample, sample_rate, number, frame_number_step,
                                                     static_cast<uint8_t*>(h->d_pack[s].ptr), cbound, dlen, h->stream);
    } else if (stereo) {
      rc = flacenc_hip_encode_pack_stereo_frames_async(
          h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), c.frames, c.n, cstride, bits_per_sample, sample_rate,
          number, frame_number_step, static_cast<flacenc_hip_stereo_frame_result*>(h->d_results.ptr),
          static_cast<uint8_t*>(h->d_pack[s].ptr), cbound, dlen, h->stream);
    } else {  // Independent(channels) frames, src/coding.rs:537-541
      rc = flacenc_hip_encode_pack_frames_async(
          h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), c.frames, channels, c.n, cstride, bits_per_sample,
          sample_rate, number, frame_number_step, static_cast<flacenc_hip_channel_result*>(h->d_results.ptr),
          static_cast<uint8_t*>(h->d_pack[s].ptr), cbound, dlen, h->stream);
    }
    if (rc != FLACENC_HIP_OK) return rc;
    uint64_t* soff = static_cast<uint64_t*>(h->d_poff[s].ptr);
    uint64_t* doff = soff + c.frames;
    uint64_t* dtotal = reinterpret_cast<uint64_t*>(dlen + ((c.frames + 1) & ~static_cast<size_t>(1)));
    HIP_TRY(h, flacenc_hip::launch_frame_offsets(dlen, static_cast<uint32_t>(c.frames), cbound, soff, doff, dtotal, h->stream));
    HIP_TRY(h, flacenc_hip::launch_place_frames(static_cast<const uint8_t*>(h->d_pack[s].ptr), soff, dlen,
                                                static_cast<uint8_t*>(h->d_cont[s].ptr), doff,
                                                static_cast<uint32_t>(c.frames), h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->pin_meta[s], dlen, c.frames * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipEventRecord(h->ev_pack[s], h->stream));
    // 3. while this chunk runs: the chunk before the previous one reaches the caller (its transfer ran
    // during this chunk's staging copy), then the previous one's transfer starts
    if (ci >= 2 && (rc = finish_out(ci - 2)) != FLACENC_HIP_OK) return rc;
    if (ci >= 1 && (rc = start_out(ci - 1)) != FLACENC_HIP_OK) return rc;
  }
  const size_t nc = chunks.size();
  if (nc >= 2 && (rc = finish_out(nc - 2)) != FLACENC_HIP_OK) return rc;
  if ((rc = start_out(nc - 1)) != FLACENC_HIP_OK) return rc;
  if ((rc = finish_out(nc - 1)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->s_out));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  drain_on_error.armed = false;
  *out_total = written;
  return FLACENC_HIP_OK;
}

}  // extern "C"
