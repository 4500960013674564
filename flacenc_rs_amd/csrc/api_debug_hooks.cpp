// api_debug_hooks.cpp -- the test and profiling hooks of flacenc_hip_debug.h and nothing else: this object is linked into
// libflacenc_hip_hooks.so only, so the product library has none of them.
#include "api_internal.h"
#include "flacenc_hip_debug.h"
#include "stream_encode_core.h"
#include "stream_index.h"

extern "C" {

int flacenc_hip_debug_scratch_bytes(flacenc_hip_handle* h, uint64_t out[2]) {
  if (!h || !out) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  out[0] = out[1] = 0;
  for (const flacenc_hip::DeviceBuffer* b : flacenc_hip::device_buffers(h)) {
    if (!b->ptr) continue;
    out[0] += b->cap;
    if (b->cap > out[1]) out[1] = b->cap;
  }
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_search_slices(flacenc_hip_handle* h, uint32_t* slices) {
  if (!h || !slices) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  *slices = h->last_search_slices;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_fixed_keys(flacenc_hip_handle* h, unsigned long long* device_keys) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->fixed_keys = device_keys;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_stamps(flacenc_hip_handle* h, unsigned long long* device_stamps) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->stamps = device_stamps;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_adaptive_order(flacenc_hip_handle* h, int on) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->adaptive.enabled = on ? 1 : 0;
  h->adaptive.state.left = h->adaptive.state.span = 0;
  h->adaptive.state.probe_out = false;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_adaptive_state(flacenc_hip_handle* h, int* span, int* left) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (span) *span = h->adaptive.state.span;
  if (left) *left = h->adaptive.state.left;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_order_guess_trace(flacenc_hip_handle* h, void* device_trace) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->order_guess_trace = device_trace;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_cert_stats(flacenc_hip_handle* h, uint32_t* device_counters) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->cert_stats = device_counters;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_stream_chunk(flacenc_hip_handle* h, size_t frames) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (frames > 8192) {  // the rule's own upper end; flacenc_hip_fill_le_bytes_async takes at most 65535 frames
    h->last_error = "debug_set_stream_chunk: more than 8192 frames per chunk";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->stream_chunk_override = frames;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_stream_plan(flacenc_hip_handle* h, size_t* chunk_frames, size_t* n_chunks) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (chunk_frames) *chunk_frames = h->last_stream_chunk;
  if (n_chunks) *n_chunks = h->last_stream_chunks;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_stream_buffers(flacenc_hip_handle* h, int* in_pinned, int* out_pinned) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (in_pinned) *in_pinned = h->last_stream_in_pinned ? 1 : 0;
  if (out_pinned) *out_pinned = h->last_stream_out_pinned ? 1 : 0;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_decode_plan(flacenc_hip_handle* h, size_t window_bytes, size_t group_frames) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (group_frames > 8192) {  // the rule's own upper end
    h->last_error = "debug_set_decode_plan: more than 8192 frames per group";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->decode_window_override = window_bytes;
  h->decode_group_override = group_frames;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_decode_plan(flacenc_hip_handle* h, size_t* window_bytes, size_t* n_windows,
                                       size_t* group_frames, size_t* n_groups) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (window_bytes) *window_bytes = h->last_decode_window;
  if (n_windows) *n_windows = h->last_decode_windows;
  if (group_frames) *group_frames = h->last_decode_group;
  if (n_groups) *n_groups = h->last_decode_groups;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_decode_streams_plan(flacenc_hip_handle* h, uint64_t plan[4]) {
  if (!h || !plan) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) plan[i] = h->last_streams_plan[i];
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_decode_ranges_plan(flacenc_hip_handle* h, uint64_t plan[4]) {
  if (!h || !plan) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) plan[i] = h->last_ranges_plan[i];
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_recover_plan(flacenc_hip_handle* h, uint64_t plan[4]) {
  if (!h || !plan) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) plan[i] = h->last_recover_plan[i];
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_encode_streams_chunk(flacenc_hip_handle* h, size_t frames) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (frames > 8192) {  // the rule's own upper end
    h->last_error = "debug_set_encode_streams_chunk: more than 8192 frames per frame-level call";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->encode_streams_chunk_override = frames;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_last_encode_streams_plan(flacenc_hip_handle* h, uint64_t plan[8]) {
  if (!h || !plan) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  for (int i = 0; i < 8; ++i) plan[i] = h->last_encode_streams_plan[i];
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_set_planar_fill_form(flacenc_hip_handle* h, int form) {
  if (!h || (form != 0 && form != 1)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->planar_fill_form = form;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_streams_fill(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples, uint32_t channels,
                                   uint32_t bytes_per_sample, size_t n_frames, uint32_t block_size, int32_t* frames,
                                   size_t stride) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!bytes || !frames || channels < 1 || channels > 8 || bytes_per_sample < 1 || bytes_per_sample > 4 ||
      block_size < 1 || block_size > FLACENC_HIP_MAX_BLOCK_SIZE || stride < block_size || (stride & 3) ||
      (reinterpret_cast<uintptr_t>(frames) & 15) || n_frames > 0x7FFFFFFFull) {
    h->last_error = "debug_streams_fill: null pointer, channels not in 1..=8, bytes_per_sample not in 1..=4, rows not "
                    "16-byte aligned, stride no multiple of 4 or below block_size, or 2^31 frames or more";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  std::vector<streamenc::LaunchFrame> table(n_frames);
  const uint64_t per = static_cast<uint64_t>(channels) * bytes_per_sample;
  for (size_t f = 0; f < n_frames; ++f) {
    const uint64_t at = static_cast<uint64_t>(f) * block_size;
    const uint64_t left = at < total_samples ? total_samples - at : 0;
    table[f] = {at * per, static_cast<uint32_t>(left < block_size ? left : block_size), static_cast<uint32_t>(f)};
  }
  HIP_TRY(h, hipSetDevice(h->device));
  int rc;
  if ((rc = flacenc_hip::ensure(h, h->d_encs, n_frames * sizeof(streamenc::LaunchFrame))) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->d_encs.ptr, table.data(), n_frames * sizeof(streamenc::LaunchFrame), hipMemcpyHostToDevice,
                            h->stream));
  HIP_TRY(h, flacenc_hip::launch_streams_fill(bytes, static_cast<const streamenc::LaunchFrame*>(h->d_encs.ptr),
                                              static_cast<uint32_t>(n_frames), channels, bytes_per_sample, 0, stride, frames,
                                              h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_segmax_scan(flacenc_hip_handle* h, const uint64_t* values, const uint8_t* heads, size_t n,
                                  size_t room, uint64_t* out) {
  using namespace flacenc_hip;
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (room < n || room > streambatch::MAX_FRAMES || (n && (!values || !heads || !out || !heads[0]))) {
    h->last_error = "debug_segmax_scan: null pointer, room below n or above 2^30, or element 0 is no head";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // the frame sequence the kernels see: segment k is slot k, base[k] its head's index, base[segments] = n
  std::vector<uint32_t> slot(n);
  std::vector<uint64_t> base;
  for (size_t m = 0; m < n; ++m) {
    if (heads[m]) base.push_back(m);
    slot[m] = static_cast<uint32_t>(base.size() - 1);
  }
  base.push_back(n);
  const uint32_t counters[4] = {0, 0, 0, static_cast<uint32_t>(n)};  // streamindex::C_FRAMES
  static_assert(streamindex::C_FRAMES == 3, "counters above");
  const size_t NB = (room + 255) / 256;
  const size_t o_emax = 0, o_base = o_emax + a256(room * 8 + 8), o_aggv = o_base + a256(base.size() * 8);
  const size_t o_slot = o_aggv + a256(NB * 8 + 8), o_aggh = o_slot + a256(n * 4 + 4), o_counters = o_aggh + a256(NB * 4 + 4);
  HIP_TRY(h, hipSetDevice(h->device));
  struct Scratch {
    char* p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } d;
  HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&d.p), o_counters + 256));
  hipStream_t st = h->stream;
  streamindex::Drain drain{h};  // the host vectors and the scratch outlive what was queued, on every way out
  uint64_t* emax = reinterpret_cast<uint64_t*>(d.p + o_emax);
  if (n) {
    HIP_TRY(h, hipMemcpyAsync(emax, values, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(d.p + o_slot, slot.data(), n * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(h, hipMemcpyAsync(d.p + o_base, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(d.p + o_counters, counters, sizeof counters, hipMemcpyHostToDevice, st));
  uint64_t plan[4] = {0, 0, 0, 0};
  const hipError_t launched = launch_segmax_scan(plan, reinterpret_cast<const uint32_t*>(d.p + o_slot),
                                                 reinterpret_cast<const uint64_t*>(d.p + o_base), emax,
                                                 reinterpret_cast<const uint32_t*>(d.p + o_counters), room,
                                                 reinterpret_cast<uint32_t*>(d.p + o_aggh),
                                                 reinterpret_cast<uint64_t*>(d.p + o_aggv), st);
  HIP_TRY(h, launched);
  if (n) HIP_TRY(h, hipMemcpyAsync(out, emax, n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  drain.armed = false;
  return FLACENC_HIP_OK;
}

}  // extern "C"
