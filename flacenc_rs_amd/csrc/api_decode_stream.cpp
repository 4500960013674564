// api_decode_stream.cpp -- the way back at the host boundary: decoded rows to packed PCM (flacenc_hip_pack_le_bytes,
// kernels: pcm_pack.cpp) and a whole stream of frames in host memory to packed PCM in host memory
// (flacenc_hip_decode_pcm), windowed and grouped over two slots of staging and three streams like api_stream.cpp.
#include "api_internal.h"
#include "flac_decode.h"
#include "pcm_pack.h"

using namespace flacenc_hip;

namespace {

int check_pack_args(flacenc_hip_handle* h, const int32_t* frames, const uint32_t* block_sizes, size_t n_frames,
                    uint32_t channels, uint32_t bytes_per_sample, const uint8_t* out, uint64_t out_capacity,
                    const uint64_t* total) {
  if (!total || (n_frames && (!frames || !block_sizes)) || (out_capacity && !out) || channels < 1 || channels > 8 ||
      bytes_per_sample < 1 || bytes_per_sample > 4 || n_frames > 0x7FFFFFFFull) {
    h->last_error = "pack_le_bytes: null pointer, channels not in 1..=8, bytes_per_sample not in 1..=4 or more than "
                    "2^31 - 1 frames";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

// The two launches of flacenc_hip_pack_le_bytes on device pointers, enqueued on `s`: what the blocking call and the
// groups of flacenc_hip_decode_pcm share.  No synchronise, no allocation once the handle's scratch has its size.
int enqueue_pack_le_bytes(flacenc_hip_handle* h, const int32_t* frames, size_t stride, const uint32_t* block_sizes,
                          size_t n_frames, uint32_t channels, uint32_t bytes_per_sample, uint8_t* out,
                          uint64_t out_capacity, uint64_t* sample_offsets, uint64_t* total, hipStream_t s) {
  int rc = check_pack_args(h, frames, block_sizes, n_frames, channels, bytes_per_sample, out, out_capacity, total);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (!sample_offsets) {
    if ((rc = ensure(h, h->d_ppk_off, (n_frames + 1) * 8)) != FLACENC_HIP_OK) return rc;
    sample_offsets = static_cast<uint64_t*>(h->d_ppk_off.ptr);
  }
  HIP_TRY(h, flacenc_hip::launch_pcm_offsets(block_sizes, n_frames, stride, sample_offsets, total, s));
  HIP_TRY(h, flacenc_hip::launch_pack_le_bytes(frames, stride, block_sizes, sample_offsets, n_frames, channels,
                                               bytes_per_sample, out, out_capacity, s));
  return FLACENC_HIP_OK;
}

}  // namespace

extern "C" {

int flacenc_hip_pack_le_bytes(flacenc_hip_handle* h, const int32_t* frames, size_t stride, const uint32_t* block_sizes,
                              size_t n_frames, uint32_t channels, uint32_t bytes_per_sample, uint8_t* out,
                              uint64_t out_capacity, uint64_t* sample_offsets, uint64_t* total, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind != FLACENC_HIP_MEM_DEVICE && memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  int rc = check_pack_args(h, frames, block_sizes, n_frames, channels, bytes_per_sample, out, out_capacity, total);
  if (rc != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  uint64_t host_total = 0;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE) {
    rc = enqueue_pack_le_bytes(h, frames, stride, block_sizes, n_frames, channels, bytes_per_sample, out,
                                         out_capacity, sample_offsets, total, s);
    if (rc != FLACENC_HIP_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(&host_total, total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
  } else {
    // host pointers: stage through the handle's device scratch, rows at the caller's stride
    const size_t row_bytes = n_frames * channels * stride * 4;
    uint64_t need = 0;  // the bytes of the output, from the caller's own block sizes
    for (size_t f = 0; f < n_frames; ++f) need += block_sizes[f] < stride ? block_sizes[f] : stride;
    need *= static_cast<uint64_t>(channels) * bytes_per_sample;
    const bool fits = need <= out_capacity;
    const size_t o_bs = a256(row_bytes), o_off = o_bs + a256(n_frames * 4), o_total = o_off + a256((n_frames + 1) * 8),
                 o_out = o_total + 256, all = o_out + (fits ? static_cast<size_t>(need) : 0) + 16;
    if ((rc = ensure(h, h->d_ppk_io, all)) != FLACENC_HIP_OK) return rc;
    char* d = static_cast<char*>(h->d_ppk_io.ptr);
    if (n_frames) {
      HIP_TRY(h, hipMemcpyAsync(d, frames, row_bytes, hipMemcpyHostToDevice, s));
      HIP_TRY(h, hipMemcpyAsync(d + o_bs, block_sizes, n_frames * 4, hipMemcpyHostToDevice, s));
    }
    rc = enqueue_pack_le_bytes(h, reinterpret_cast<const int32_t*>(d), stride,
                                         reinterpret_cast<const uint32_t*>(d + o_bs), n_frames, channels,
                                         bytes_per_sample, reinterpret_cast<uint8_t*>(d + o_out), out_capacity,
                                         reinterpret_cast<uint64_t*>(d + o_off),
                                         reinterpret_cast<uint64_t*>(d + o_total), s);
    if (rc != FLACENC_HIP_OK) return rc;
    if (sample_offsets) HIP_TRY(h, hipMemcpyAsync(sample_offsets, d + o_off, (n_frames + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(&host_total, d + o_total, 8, hipMemcpyDeviceToHost, s));
    if (fits && need) HIP_TRY(h, hipMemcpyAsync(out, d + o_out, need, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    total[0] = host_total;
  }
  if (host_total * channels * bytes_per_sample > out_capacity) {
    h->last_error = "pack_le_bytes: out_capacity too small";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

int flacenc_hip_decode_pcm(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, uint32_t channels,
                           uint32_t bits_per_sample, uint32_t max_block_size, uint32_t bytes_per_sample, uint8_t* out,
                           uint64_t out_capacity, uint64_t totals[4]) {
  if (!h || !totals) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  totals[0] = totals[1] = totals[2] = totals[3] = 0;
  // flacenc_hip_debug_last_decode_plan: no window has run yet
  h->last_decode_window = h->last_decode_windows = h->last_decode_group = h->last_decode_groups = 0;
  if (channels < 1 || channels > 8 || max_block_size < 1 || max_block_size > 65536 || bytes_per_sample > 4 ||
      (n_bytes && !bytes) || (out_capacity && !out)) {
    h->last_error = "decode_pcm: null pointer, channels not in 1..=8, max_block_size not in 1..=65536 or "
                    "bytes_per_sample above 4";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (bits_per_sample < 4 || bits_per_sample > h->max_bps) {
    h->last_error = "decode_pcm: bits_per_sample not in 4..=24 (4..=32 with flacenc_hip_set_max_bits_per_sample)";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  if (bytes_per_sample < (bits_per_sample + 7) / 8) {
    h->last_error = "decode_pcm: bytes_per_sample below ceil(bits_per_sample / 8)";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (n_bytes == 0) return FLACENC_HIP_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  if ((rc = ensure_stream_objects(h)) != FLACENC_HIP_OK) return rc;

  // ---- the plan ----
  // B: no frame of the stream is longer (every frame the library's encoders write; a longer one ends the chain).
  // Windows of W >= 2B input bytes on a fixed grid that advances by W - B: the chain found in a window ends inside its
  // last B bytes, so the next window -- uploaded without waiting for this one's index -- holds the next frame start.
  size_t B = flacenc_hip_frame_bytes_bound(channels, max_block_size, bits_per_sample);
  if (channels == 2) {
    const size_t sb = flacenc_hip_stereo_frame_bytes_bound(max_block_size, bits_per_sample);
    if (sb > B) B = sb;
  }
  uint64_t W = static_cast<uint64_t>(128) << 20;
  // (test hook flacenc_hip_debug_set_decode_plan, hooks library only: seams after a handful of frames)
  if (h->decode_window_override) W = h->decode_window_override;
  if (W < 2 * B) W = 2 * B;
  const uint64_t step = W - B;
  const size_t w_room = static_cast<size_t>(W < n_bytes ? W : n_bytes);  // bytes a window slot holds
  // Groups of whole frames bound the rows and the PCM staging: a window of digital silence decodes to a thousand times
  // its bytes, so nothing on the output side is sized from input bytes.  The decoder walks a frame on one lane, so a
  // launch takes as long for a hundred frames as for a hundred thousand: the group is what sets
  // the call's rate, and the budget buys as many frames per launch as the staging can reasonably hold.
  const size_t frame_pcm = static_cast<size_t>(max_block_size) * channels * bytes_per_sample;
  size_t group = (static_cast<size_t>(128) << 20) / frame_pcm;
  group = group < 64 ? 64 : (group > 8192 ? 8192 : group);
  if (h->decode_group_override) group = h->decode_group_override;
  const uint64_t most_frames = n_bytes / 9 + 1;  // a frame is at least 9 bytes: never more staging than the call can use
  if (group > most_frames) group = static_cast<size_t>(most_frames);
  // frames one index launch can return; a window that holds more is indexed again from where the chain stopped
  size_t idx_frames = w_room / 9 + 1;
  if (idx_frames > 32768) idx_frames = 32768;
  const size_t dstride = padded_stride(max_block_size);
  const size_t meta_bytes = 8 + group * 16;  // total | frame offsets | status | block sizes: one copy per group
  const bool in_pinned = is_pinned(bytes), out_pinned = out_capacity == 0 || is_pinned(out);
  if (!in_pinned && (rc = ensure_pinned(h, h->pin_in, &h->pin_in_cap, w_room)) != FLACENC_HIP_OK) return rc;
  // (a group's transfer never exceeds what `out` still holds)
  const uint64_t out_stage = group * frame_pcm < out_capacity ? group * frame_pcm : out_capacity;
  if (!out_pinned && (rc = ensure_pinned(h, h->pin_out, &h->pin_out_cap, static_cast<size_t>(out_stage))) != FLACENC_HIP_OK)
    return rc;
  if ((rc = ensure_pinned(h, h->pin_meta, &h->pin_meta_cap, meta_bytes)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_samples, group * channels * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_dec, flacenc_hip::decode_scratch_bytes(group))) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_idx, flacenc_hip::index_scratch_bytes(w_room, flacenc_hip::index_candidate_capacity(idx_frames)))) != FLACENC_HIP_OK)
    return rc;
  if ((rc = ensure(h, h->d_dpcm_idx, a256(idx_frames * 8) + a256(idx_frames * 4) + 256)) != FLACENC_HIP_OK) return rc;
  for (int i = 0; i < 2; ++i) {
    if ((rc = ensure(h, h->d_pcm[i], w_room + 16)) != FLACENC_HIP_OK) return rc;           // a window's bytes
    if ((rc = ensure(h, h->d_cont[i], group * frame_pcm + 16)) != FLACENC_HIP_OK) return rc;  // a group's PCM
    if ((rc = ensure(h, h->d_plen[i], meta_bytes)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_poff[i], (group + 1) * 8)) != FLACENC_HIP_OK) return rc;        // sample offsets
  }
  if ((!in_pinned || !out_pinned) && (rc = ensure_copy_pool(h, "decode_pcm")) != FLACENC_HIP_OK) return rc;
  uint64_t* d_off = static_cast<uint64_t*>(h->d_dpcm_idx.ptr);
  uint32_t* d_len = reinterpret_cast<uint32_t*>(static_cast<char*>(h->d_dpcm_idx.ptr) + a256(idx_frames * 8));
  uint64_t* d_cnt = reinterpret_cast<uint64_t*>(static_cast<char*>(h->d_dpcm_idx.ptr) + a256(idx_frames * 8) + a256(idx_frames * 4));
  h->last_decode_window = static_cast<size_t>(W);
  h->last_decode_group = group;

  // ---- the way out, one group behind the way in (api_stream.cpp's start_out / finish_out) ----
  uint64_t frames_done = 0, samples_done = 0, written = 0;
  bool stopped = false;  // a frame with a status, or no room: nothing behind it reaches the caller
  uint64_t stop_at = 0, stop_why = 0;
  struct Slot {
    uint64_t base = 0;  // stream position the group's frame offsets count from
    size_t n = 0;
    uint64_t at = 0, bytes = 0;  // the transfer finish_out hands over
  } slot[2];
  auto start_out = [&](size_t gi) -> int {
    Slot& g = slot[gi & 1];
    const int s = static_cast<int>(gi & 1);
    g.bytes = 0;
    HIP_TRY(h, hipEventSynchronize(h->ev_pack[s]));  // the group's records are in pin_meta[s]
    if (stopped) return FLACENC_HIP_OK;
    const char* m = static_cast<const char*>(h->pin_meta[s]);
    const uint64_t* offs = reinterpret_cast<const uint64_t*>(m + 8);
    const uint32_t* st = reinterpret_cast<const uint32_t*>(m + 8 + g.n * 8);
    const uint32_t* bs = st + g.n;
    uint64_t bytes = 0;
    for (size_t j = 0; j < g.n && !stopped; ++j) {
      const uint64_t fb = static_cast<uint64_t>(bs[j]) * channels * bytes_per_sample;
      if (st[j]) {
        stop_why = st[j];
      } else if (fb > out_capacity - written - bytes) {
        stop_why = FLACENC_HIP_DECODE_NO_ROOM;
      } else {
        bytes += fb;
        samples_done += bs[j];
        ++frames_done;
        continue;
      }
      stopped = true;
      stop_at = g.base + offs[j];
    }
    if (bytes)
      HIP_TRY(h, hipMemcpyAsync(out_pinned ? static_cast<void*>(out + written) : h->pin_out[s], h->d_cont[s].ptr, bytes,
                                hipMemcpyDeviceToHost, h->s_out));
    HIP_TRY(h, hipEventRecord(h->ev_d2h[s], h->s_out));
    g.at = written;
    g.bytes = bytes;
    written += bytes;
    return FLACENC_HIP_OK;
  };
  auto finish_out = [&](size_t gi) -> int {
    const Slot& g = slot[gi & 1];
    if (out_pinned || g.bytes == 0) return FLACENC_HIP_OK;
    HIP_TRY(h, hipEventSynchronize(h->ev_d2h[gi & 1]));
    h->copy_pool->copy(out + g.at, h->pin_out[gi & 1], g.bytes);
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

  // window k = bytes [k * step, k * step + W) of the input, in slot k & 1
  auto upload = [&](uint64_t k) -> int {
    const uint64_t ws = k * step, we = ws + W < n_bytes ? ws + W : n_bytes;
    const int s = static_cast<int>(k & 1);
    const size_t len = static_cast<size_t>(we - ws);
    if (k >= 2) HIP_TRY(h, hipStreamWaitEvent(h->s_in, h->ev_fill[s], 0));  // window k - 2 has been decoded
    if (in_pinned) {
      HIP_TRY(h, hipMemcpyAsync(h->d_pcm[s].ptr, bytes + ws, len, hipMemcpyHostToDevice, h->s_in));
    } else {
      if (k >= 2) HIP_TRY(h, hipEventSynchronize(h->ev_h2d[s]));  // pin_in[s] has been sent
      h->copy_pool->copy(h->pin_in[s], bytes + ws, len);
      HIP_TRY(h, hipMemcpyAsync(h->d_pcm[s].ptr, h->pin_in[s], len, hipMemcpyHostToDevice, h->s_in));
    }
    HIP_TRY(h, hipEventRecord(h->ev_h2d[s], h->s_in));
    return FLACENC_HIP_OK;
  };

  uint64_t cur = 0;       // where the next frame of the chain starts
  uint64_t end_why = 0;   // why the chain itself ended: 0 (at n_bytes) or CHAIN
  size_t issued = 0;      // groups
  bool done = false;
  if ((rc = upload(0)) != FLACENC_HIP_OK) return rc;
  for (uint64_t k = 0; !done; ++k) {
    const uint64_t ws = k * step, we = ws + W < n_bytes ? ws + W : n_bytes;
    const bool last = we == n_bytes;
    const int ws_slot = static_cast<int>(k & 1);
    h->last_decode_windows = static_cast<size_t>(k + 1);
    if (!last && (rc = upload(k + 1)) != FLACENC_HIP_OK) return rc;  // before this window's index is known
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_h2d[ws_slot], 0));
    for (;;) {
      // the verified chain from `cur` as far as this window holds it (INDEX_ERROR is the rule here: the window cuts a
      // frame, or holds more than idx_frames)
      const uint64_t avail = we - cur;
      const uint8_t* base = static_cast<const uint8_t*>(h->d_pcm[ws_slot].ptr) + (cur - ws);
      uint64_t count = 0;
      rc = flacenc_hip_index_frames_async(h, base, avail, channels, bits_per_sample, idx_frames, d_off, d_len, d_cnt,
                                          h->stream);
      if (rc != FLACENC_HIP_OK) return rc;
      HIP_TRY(h, hipMemcpyAsync(&count, d_cnt, 8, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      const size_t nf = static_cast<size_t>(count & ~FLACENC_HIP_INDEX_ERROR);
      if (nf == 0) {
        // a whole frame would have fitted (or the input ends here) and none verifies: the chain is broken at `cur`
        if (last || avail >= B) {
          end_why = FLACENC_HIP_DECODE_CHAIN;
          done = true;
        }
        break;
      }
      uint64_t last_off = 0;
      uint32_t last_len = 0;
      HIP_TRY(h, hipMemcpyAsync(&last_off, d_off + (nf - 1), 8, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(&last_len, d_len + (nf - 1), 4, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      // groups of at most `group` frames, cut evenly so that none is a small remainder
      const size_t parts = (nf + group - 1) / group, per = (nf + parts - 1) / parts;
      for (size_t f0 = 0; f0 < nf && !stopped; f0 += per) {
        const size_t n = nf - f0 < per ? nf - f0 : per;
        const size_t gi = issued;
        const int s = static_cast<int>(gi & 1);
        if (gi >= 2) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_d2h[s], 0));  // d_cont[s] has been copied out
        char* meta = static_cast<char*>(h->d_plen[s].ptr);
        uint64_t* m_total = reinterpret_cast<uint64_t*>(meta);
        uint64_t* m_off = reinterpret_cast<uint64_t*>(meta + 8);
        uint32_t* m_st = reinterpret_cast<uint32_t*>(meta + 8 + n * 8);
        uint32_t* m_bs = m_st + n;
        rc = flacenc_hip_decode_frames_async(h, base, d_off + f0, d_len + f0, n, channels, bits_per_sample,
                                             max_block_size, static_cast<int32_t*>(h->d_samples.ptr), dstride, m_bs,
                                             nullptr, m_st, h->stream);
        if (rc != FLACENC_HIP_OK) return rc;
        rc = enqueue_pack_le_bytes(h, static_cast<const int32_t*>(h->d_samples.ptr), dstride, m_bs, n, channels,
                                             bytes_per_sample, static_cast<uint8_t*>(h->d_cont[s].ptr), group * frame_pcm,
                                             static_cast<uint64_t*>(h->d_poff[s].ptr), m_total, h->stream);
        if (rc != FLACENC_HIP_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(m_off, d_off + f0, n * 8, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->pin_meta[s], meta, 8 + n * 16, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipEventRecord(h->ev_pack[s], h->stream));
        slot[s].base = cur;
        slot[s].n = n;
        ++issued;
        // while this group runs: the group before the previous one reaches the caller, the previous one's transfer starts
        if (gi >= 2 && (rc = finish_out(gi - 2)) != FLACENC_HIP_OK) return rc;
        if (gi >= 1 && (rc = start_out(gi - 1)) != FLACENC_HIP_OK) return rc;
      }
      if (stopped) {
        done = true;
        break;
      }
      cur += last_off + last_len;
      if (cur == n_bytes) {
        done = true;  // the chain ended exactly at n_bytes
        break;
      }
      if (!last && we - cur < B) break;  // the next frame start lies in the next window's first B bytes
      // else: the chain stopped with room for a whole frame behind it (idx_frames reached, a full candidate table, or
      // a broken frame): index again from there, and zero frames is then the CHAIN stop
    }
    HIP_TRY(h, hipEventRecord(h->ev_fill[ws_slot], h->stream));  // the slot's bytes have been read
  }
  h->last_decode_groups = issued;
  if (issued >= 2 && (rc = finish_out(issued - 2)) != FLACENC_HIP_OK) return rc;
  if (issued >= 1) {
    if ((rc = start_out(issued - 1)) != FLACENC_HIP_OK) return rc;
    if ((rc = finish_out(issued - 1)) != FLACENC_HIP_OK) return rc;
  }
  HIP_TRY(h, hipStreamSynchronize(h->s_in));  // (a window uploaded ahead of a stop reads the caller's bytes)
  HIP_TRY(h, hipStreamSynchronize(h->s_out));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  drain_on_error.armed = false;
  totals[0] = frames_done;
  totals[1] = samples_done;
  totals[2] = stopped ? stop_at : cur;
  totals[3] = stopped ? stop_why : end_why;
  return FLACENC_HIP_OK;
}

}  // extern "C"
