// frame_plan.h -- what a frame-level call does, decided in one pure step ("The plan of a frame-level call"):
// the launch records' config-derived fields, the scratch rule, and the path of the call as a value.  No HIP call, nothing
// allocated, no handle: compiles for the host alone next to qlpc_dispatch.cpp (tests/host/frame_plan_test.cpp).
#ifndef FLACENC_HIP_FRAME_PLAN_H_
#define FLACENC_HIP_FRAME_PLAN_H_

#include "qlpc_kernel.h"

namespace flacenc_hip {

// The LPC candidate of a (normalised) config comes from the search over windows, orders and precisions (order_search.h)
bool lpc_search(uint32_t flags);
// FLACENC_HIP_FLAG_WINDOW_SEARCH with no extra window is exactly the call with the summation-order flag in its place
// (with FLACENC_HIP_FLAG_ORDER_SEARCH: the ORDER_SEARCH call; with FLACENC_HIP_FLAG_ORDER_GUESS: the ORDER_GUESS call),
// and so is FLACENC_HIP_FLAG_PRECISION_SEARCH with the handle's floor at or above the config's quant_precision.
uint32_t search_flags(bool extra_windows, uint32_t precision_floor, uint32_t flags, uint32_t quant_precision);

// ---- the launch records, as far as the config and the shape decide them ----
// What every launch record shares: the rows, order and precision, max_rice_parameter, the flag-derived words
// (force_generic, reference_order, certify, integer_parity_only) and direct_mse.  The callers add window, outputs, hooks.
QlpcKernelArgs config_record(const flacenc_hip_qlpc_config& q, const int32_t* samples, size_t stride, uint32_t block_size,
                             size_t n_subframes, const uint8_t* bps, uint32_t bps_uniform, bool stereo);
// ... of the fixed_lpc batch (no window, no quantisation; fixed_mode 1 under ApproxEnt, else left to the BitCount loop)
void fixed_batch_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg);
// ... of a frame-level launch (encode_frame's switches; the caller names frame_results / chan_results)
void frame_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg, bool stereo, uint32_t group_log2);
// ... of the sub-wave frame kernel, from the frame-level record
void subwave_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg, uint32_t cert_subwave);

// ---- the scratch rule ----
enum class LaunchKind { kLpcBatch, kFixedBatch, kFrame, kSubwaveFrames };
struct ScratchGrant {
  bool split;   // R[] and the predictor records between the launches of a route, and the marked counters
  bool sumabs;  // sumabs_reference_kernel's per-partition sums
};
// Whether the record of a launch of `kind` is given each scratch (`search`: read for an LPC batch, a search flag is set).
// A launched record the rule denies the split scratch routes the same with and without one.
ScratchGrant scratch_grant(const QlpcKernelArgs& a, LaunchKind kind, bool search = false);

// ---- the plan ----
struct FrameCall {
  flacenc_hip_frame_config cfg;  // verified, as the caller gave it
  bool stereo;                   // 2-channel frames with the stereo decision; else Independent(n) frames
  uint32_t block_size, bits_per_sample;
  const int32_t* samples;        // the rows: only their alignment is read
  size_t stride;
  const int32_t* residual;
  size_t residual_stride;
  bool pack;                     // a pack target whose bit buffer fits the fused kernel
  bool extra_windows;            // the handle holds extra LPC windows
  uint32_t precision_floor;      // ... and this precision floor
};
struct FramePlan {  // in run order
  flacenc_hip_frame_config cfg;  // normalised: search_flags, and too_short (coding.rs:396): Constant or Verbatim
  bool search_or_escape;         // a search flag with use_lpc, or RICE_ESCAPE: the candidate batches for every shape
  uint32_t group_log2;           // QlpcKernelArgs::fixed_group_log2 of the fused kernels
  bool frame_record;             // the frame-level record is built and given its scratch (kFrame)
  bool fused_pack;               // ... with the bit writer (kFused only)
  enum Path : uint8_t { kGeneral, kFused, kBigBlock, kSubwave } path;
  bool subwave_scratch;          // the sub-wave record is built and given its scratch (kSubwaveFrames), taken or not
  uint32_t cert_subwave;
  bool lpc_batch, fixed_batch;   // the candidate batches that run (kSubwave: as clean-ups of what the kernel marked)
};
FramePlan plan_frame_call(const FrameCall& call);
// The record the plan asks the eligibility predicates about -- what the call will launch, with placeholders for outputs
// and scratch: kFrame (before its scratch is granted), kLpcBatch or kFixedBatch
QlpcKernelArgs probe_record(const FrameCall& call, const FramePlan& plan, LaunchKind kind);

inline size_t padded_stride(uint32_t block_size) { return (static_cast<size_t>(block_size) + 3) & ~static_cast<size_t>(3); }

}  // namespace flacenc_hip
#endif
