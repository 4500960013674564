/* flacenc_hip_debug.h -- test and profiling hooks.  NOT part of the drop-in boundary (include/flacenc_hip.h) and NOT in
 * the product library: they are api_debug_hooks.cpp, whose object the Makefile leaves out of libflacenc_hip.so and links
 * into a second library, libflacenc_hip_hooks.so -- otherwise the same objects -- for tests/ and tools/
 * (flacenc_rs_amd/_capi.py: Handle(dev, hooks=True)). */
#ifndef FLACENC_HIP_DEBUG_H_
#define FLACENC_HIP_DEBUG_H_

#include "flacenc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook (no reference counterpart): when `device_keys` is non-NULL, launches with use_fixed
 * store the order selector's key for each tried fixed order (estimate_entropy + bps*order, or
 * the BitCount bits; src/coding.rs:249, :271) at device_keys[subframe*8 + order]. */
int flacenc_hip_debug_set_fixed_keys(flacenc_hip_handle* h, unsigned long long* device_keys);

/* Test hook (no reference counterpart): when `device_trace` is non-NULL, every launch of the search under
 * FLACENC_HIP_FLAG_ORDER_GUESS stores what order_guess_kernel computed for each (subframe, window) -- the guess itself,
 * which otherwise never leaves the handle's scratch -- as one record of 264 bytes,
 *   uint32 eligible;   orders 1..eligible are eligible
 *   uint32 mask;       bit o - 1: order o is one of the window's guesses
 *   double cost[32];   cost[o - 1] of order o <= eligible, +0.0 in every entry above
 * at record index sf * W + j: sf the subframe of the call (not of a slice of it; stereo calls: 4 * frame + role), j the
 * window, W the number of windows the call searches (1 without FLACENC_HIP_FLAG_WINDOW_SEARCH or with an empty
 * extra-window list, else 1 + the handle's extra windows).  The caller sizes the buffer: subframes * W records.  A call
 * that launches the search more than once (flacenc_hip_encode_variable; with FLACENC_HIP_FLAG_WASTED_BITS the pass
 * over every frame, left out when every frame has wasted bits, and then the fix-up of the marked frames' shifted rows)
 * overwrites the buffer: every launch counts its own subframes from 0.  Calls without the flag store nothing.  Pass NULL to switch it off again. */
int flacenc_hip_debug_set_order_guess_trace(flacenc_hip_handle* h, void* device_trace);

/* Profiling hook (no reference counterpart): when `device_stamps` is non-NULL every
 * following launch makes each workgroup leader store 8 shader-clock timestamps
 * (phase boundaries of the fused kernel) at device_stamps[subframe*8 + phase].
 * Pass NULL to switch it off again.  See tools/phase_profile.py. */
int flacenc_hip_debug_set_stamps(flacenc_hip_handle* h, unsigned long long* device_stamps);

/* Statistics hook (no reference counterpart): when `device_counters` is non-NULL (3 x uint32, zeroed by the caller),
 * launches that certify their summation order (blocks of 4096 / 4608 samples, orders up to 12, no order flag) add to
 * [0] the subframes analysed, [1] the certificates that needed the rows of the inverse Toeplitz matrix, [2] the subframes
 * recomputed from the reference's chains. */
int flacenc_hip_debug_set_cert_stats(flacenc_hip_handle* h, uint32_t* device_counters);
/* 0: launches of the certified shapes always take the fused kernel's certificate; 1 (default): integer-only launches of
 * any size take the two-pass form (the reference's chains for every subframe, same integers) while the
 * certificate's counters of the launches before them say the material is hard (api_candidates.cpp, launch_adaptive) */
int flacenc_hip_debug_set_adaptive_order(flacenc_hip_handle* h, int on);
/* the current span of two-pass launches (0: the material last seen was easy) and how many of it are left */
int flacenc_hip_debug_adaptive_state(flacenc_hip_handle* h, int* span, int* left);

/* Test hook (no reference counterpart): the chunk plan of the streaming host path.  `frames` != 0: the calls of
 * flacenc_hip_encode_pcm / _stereo that follow cut their full blocks into chunks of `frames` frames in place of the rule
 * clamp(48 MiB / frame bytes, 768, 8192); a call with fewer full blocks than that still runs them as one chunk, and the
 * short last block stays a chunk of its own.  The bytes a call returns do not depend on the plan; the hook brings chunk
 * seams and the reuse of the two staging slots down to a handful of frames.  0 (a fresh handle): the rule.  More than
 * 8192 is FLACENC_HIP_ERR_BAD_ARGUMENT. */
int flacenc_hip_debug_set_stream_chunk(flacenc_hip_handle* h, size_t frames);
/* The plan the last flacenc_hip_encode_pcm / _stereo call on the handle ran: frames per chunk of full blocks (after the
 * cut to the call's own full blocks; 1 when it had none) and the number of chunks, the short last block's included.
 * A call that ran no chunk (total_samples == 0, rejected arguments) leaves 0 and 0.  Either pointer may be NULL. */
int flacenc_hip_debug_last_stream_plan(flacenc_hip_handle* h, size_t* chunk_frames, size_t* n_chunks);
/* How the last flacenc_hip_encode_pcm / _stereo call that got as far as its plan took the caller's buffers: 1 when it
 * found `pcm` (`out`) page-locked and transferred it directly -- a pointer into the interior of such an allocation
 * included --, 0 when it staged it through the handle's pinned slots.  Either pointer may be NULL. */
int flacenc_hip_debug_last_stream_buffers(flacenc_hip_handle* h, int* in_pinned, int* out_pinned);

/* Test hook (no reference counterpart): the plan of flacenc_hip_decode_pcm.  window_bytes != 0: the calls that follow
 * cut their input into windows of that many bytes in place of the rule (128 MiB); a value below 2B, B =
 * flacenc_hip_frame_bytes_bound(channels, max_block_size, bits_per_sample) (for 2 channels the larger of that and
 * flacenc_hip_stereo_frame_bytes_bound), is raised to 2B by the call.  group_frames != 0: they decode and pack groups of
 * that many frames in place of the rule clamp(128 MiB / (max_block_size*channels*bytes_per_sample), 64, 8192).  The bytes a
 * call returns and its totals do not depend on the plan; the hook brings window edges, group seams and the reuse of the
 * two slots down to a handful of frames.  0 (a fresh handle): the rule.  More than 8192 frames is
 * FLACENC_HIP_ERR_BAD_ARGUMENT. */
int flacenc_hip_debug_set_decode_plan(flacenc_hip_handle* h, size_t window_bytes, size_t group_frames);
/* The plan the last flacenc_hip_decode_pcm call on the handle ran: the window size in bytes and the windows it indexed,
 * the frames per group (after the cut to what the call's bytes can hold) and the groups it decoded.  A call that ran
 * no window (n_bytes == 0, rejected arguments) leaves zeros.  Any pointer may be NULL. */
int flacenc_hip_debug_last_decode_plan(flacenc_hip_handle* h, size_t* window_bytes, size_t* n_windows,
                                       size_t* group_frames, size_t* n_groups);
/* What the last flacenc_hip_decode_streams (or flacenc_hip_decode_streams_md5) call on the handle did: plan[0] kernel launches, plan[1] host
 * synchronisations, plan[2] host-device transfers, plan[3] channel counts present in its table.  None of the first three
 * depends on the number of streams.  Zeros after a call that was rejected or had no stream. */
int flacenc_hip_debug_last_decode_streams_plan(flacenc_hip_handle* h, uint64_t plan[4]);
/* What the last flacenc_hip_decode_ranges call on the handle did: plan[0] kernel launches, plan[1] host synchronisations,
 * plan[2] host-device transfers, plan[3] channel counts present among the streams its ranges name.  None of the first
 * three depends on the number of streams or of ranges; every further channel count adds one launch.  Zeros after a call
 * that was rejected or had no range. */
int flacenc_hip_debug_last_decode_ranges_plan(flacenc_hip_handle* h, uint64_t plan[4]);
/* What the last flacenc_hip_recover_streams call on the handle did: plan[0] kernel launches, plan[1] host
 * synchronisations, plan[2] host-device transfers, plan[3] channel counts present in its table.  None of the first three
 * depends on the number of streams or on the damage they hold.  Zeros after a call that was rejected or had no stream. */
int flacenc_hip_debug_last_recover_plan(flacenc_hip_handle* h, uint64_t plan[4]);

/* Test hook (no reference counterpart): the plan of flacenc_hip_encode_streams.  `frames` != 0: the calls that follow cut
 * every run of a class -- its full blocks, and the last blocks of one length -- into frame-level calls of at most `frames`
 * frames in place of the rule clamp(48 MiB / frame bytes, 768, 8192).  The bytes a call returns do not depend on the plan;
 * the hook brings the seams between frame-level calls down to a handful of frames.  0 (a fresh handle): the rule.  More
 * than 8192 is FLACENC_HIP_ERR_BAD_ARGUMENT. */
int flacenc_hip_debug_set_encode_streams_chunk(flacenc_hip_handle* h, size_t frames);
/* What the last flacenc_hip_encode_streams call on the handle did: plan[0] launches of the call's own kernels (fill,
 * lengths, scans, cut, place), plan[1] host synchronisations, plan[2] host-device transfers, plan[3] classes present in
 * its table, plan[4] full-frame runs, plan[5] tail runs, plan[6] frame-level calls (= plan[4] + plan[5]; each enqueues
 * what flacenc_hip_encode_pack_stereo_frames_async resp. flacenc_hip_encode_pack_frames_async enqueues for its shape),
 * plan[7] 0.  plan[1] and plan[2] do not depend on the number of streams; plan[0] depends on the classes only.  Zeros
 * after a call that was rejected or had no stream.  flacenc_hip_encode_streams_planar reports here too: the same words
 * for the same table, but that plan[0] also counts the launches its digests cost and plan[7] is their number (2: the
 * packed image and the hash; 1 where the table holds no frame; 0 with digests == NULL). */
int flacenc_hip_debug_last_encode_streams_plan(flacenc_hip_handle* h, uint64_t plan[8]);
/* Measurement hook (no reference counterpart): how the fill kernel of flacenc_hip_encode_streams_planar loads its
 * elements in the calls that follow: 1 (a fresh handle; what the product library always does) aligned 16-byte loads
 * brought into place, 0 four dword loads per channel.  The bytes a call returns do not depend on it. */
int flacenc_hip_debug_set_planar_fill_form(flacenc_hip_handle* h, int form);
/* Test and profiling hook (no reference counterpart): the fill kernel of flacenc_hip_encode_streams on its own, with the
 * arguments and the result of flacenc_hip_fill_le_bytes on device pointers -- `bytes` (any byte alignment) holds
 * total_samples inter-channel samples of one stream, frame f gets samples [f*block_size, (f+1)*block_size) and zeros
 * beyond total_samples -- except that `frames` must be 16-byte aligned and `stride` a multiple of 4 (rows are written up
 * to the stride, not up to block_size), and that n_frames is bounded by 2^31 - 1, not by 65535.  Builds the frame table
 * on the host, uploads it, launches once on the handle's stream and blocks. */
int flacenc_hip_debug_streams_fill(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples, uint32_t channels,
                                   uint32_t bytes_per_sample, size_t n_frames, uint32_t block_size, int32_t* frames,
                                   size_t stride);
/* Test hook (no reference counterpart): the segmented inclusive max-scan of flacenc_hip_recover_streams on its own -- the
 * same three launches (a workgroup's aggregate, one workgroup over the aggregates, the aggregates applied) the call
 * makes, sized by `room` as the call sizes them by max_frames and not by the frames it finds.  values[0 .. n) and
 * heads[0 .. n) are host memory; heads[m] != 0 makes element m the first of a segment (a stream's first chain frame).
 * out[m] (host memory, n words) gets the unsigned maximum of values from the head of m's segment up to m.  The contract:
 * element 0 is a head, as it always is in the call; room >= n, at most 2^30; anything else is
 * FLACENC_HIP_ERR_BAD_ARGUMENT.  n == 0 runs the launches over no element.  Builds the frame sequence (one slot per
 * segment) on the host, uploads it into scratch of its own, launches on the handle's stream and blocks until `out` is
 * written. */
int flacenc_hip_debug_segmax_scan(flacenc_hip_handle* h, const uint64_t* values, const uint8_t* heads, size_t n,
                                  size_t room, uint64_t* out);
/* Test hook (no reference counterpart): the device buffers the handle holds right now -- its scratch, staging and
 * tables; not the window cache, not pinned host memory.  out[0] gets the sum of their capacities in bytes, out[1] the
 * largest one's.  A buffer only ever grows (by a quarter more than was asked for), so after a call both words are at
 * least what that call needed.  tests/test_gpu_launch_scale.py asserts with it that a launch it calls large did put
 * handle scratch beyond the 2^32-byte or 2^31-element offset it claims. */
int flacenc_hip_debug_scratch_bytes(flacenc_hip_handle* h, uint64_t out[2]);
/* Test hook (no reference counterpart): into how many slices of at most kSearchScratchCap bytes of scratch the last
 * launch under FLACENC_HIP_FLAG_ORDER_SEARCH / _WINDOW_SEARCH / _ORDER_GUESS / _PRECISION_SEARCH on the handle cut its
 * subframes (order_search.cpp, slice_subframes); 0 before the first such launch. */
int flacenc_hip_debug_last_search_slices(flacenc_hip_handle* h, uint32_t* slices);

#ifdef __cplusplus
}
#endif
#endif /* FLACENC_HIP_DEBUG_H_ */
