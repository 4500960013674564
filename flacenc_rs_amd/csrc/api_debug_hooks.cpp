// api_debug_hooks.cpp -- the test and profiling hooks of flacenc_hip_debug.h and nothing else: this object is linked into
// libflacenc_hip_hooks.so only, so the product library has none of them.
#include "api_internal.h"
#include "flacenc_hip_debug.h"

extern "C" {

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
  h->adaptive_order = on ? 1 : 0;
  h->two_pass_left = h->two_pass_span = 0;
  h->fb_probe_out = false;
  return FLACENC_HIP_OK;
}

int flacenc_hip_debug_adaptive_state(flacenc_hip_handle* h, int* span, int* left) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (span) *span = h->two_pass_span;
  if (left) *left = h->two_pass_left;
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

}  // extern "C"
