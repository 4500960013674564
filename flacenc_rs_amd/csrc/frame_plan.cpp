// frame_plan.cpp -- see frame_plan.h.  Pure: every function here maps values to values.
#include "frame_plan.h"

namespace flacenc_hip {

bool lpc_search(uint32_t flags) {
  return (flags & (FLACENC_HIP_FLAG_ORDER_SEARCH | FLACENC_HIP_FLAG_WINDOW_SEARCH | FLACENC_HIP_FLAG_ORDER_GUESS |
                   FLACENC_HIP_FLAG_PRECISION_SEARCH)) != 0;
}

uint32_t search_flags(bool extra_windows, uint32_t precision_floor, uint32_t flags, uint32_t quant_precision) {
  const uint32_t dropped =
      (((flags & FLACENC_HIP_FLAG_WINDOW_SEARCH) && !extra_windows) ? FLACENC_HIP_FLAG_WINDOW_SEARCH : 0u) |
      (((flags & FLACENC_HIP_FLAG_PRECISION_SEARCH) && precision_floor >= quant_precision)
           ? FLACENC_HIP_FLAG_PRECISION_SEARCH : 0u);
  if (!dropped) return flags;
  flags &= ~dropped;
  if (lpc_search(flags)) return flags;
  flags &= ~(FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY);
  if (!(flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER)) flags |= FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER;
  return flags;
}

QlpcKernelArgs config_record(const flacenc_hip_qlpc_config& q, const int32_t* samples, size_t stride, uint32_t block_size,
                             size_t n_subframes, const uint8_t* bps, uint32_t bps_uniform, bool stereo) {
  QlpcKernelArgs a;
  a.samples = samples;
  a.stride = stride;
  a.block_size = block_size;
  a.n_subframes = static_cast<uint32_t>(n_subframes);
  a.bps = bps;
  a.bps_uniform = bps_uniform;
  a.stereo = stereo ? 1u : 0u;
  a.lpc_order = q.lpc_order;
  a.precision = q.quant_precision;
  a.max_rice_parameter = q.max_rice_parameter;
  a.rice_finest_only = (q.flags & FLACENC_HIP_FLAG_FINEST_RICE_ORDER) ? 1u : 0u;
  a.force_generic = (q.flags & FLACENC_HIP_FLAG_GENERIC_KERNEL) ? 1u : 0u;
  // reference_order: 0 = the kernels' canonical sums, 1 = the stable build's orders (FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER),
  // 2 = the simd-nightly build's (FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER)
  a.reference_order = (q.flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER) ? 2u : ((q.flags & FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER) ? 1u : 0u);
  // The unflagged order on the fused kernel's shapes is certified (QlpcKernelArgs::certify; launch_qlpc decides where it
  // applies).  Launches that cannot run it inside the fused kernel -- unaligned rows, FLACENC_HIP_FLAG_GENERIC_KERNEL, the
  // fused bit writer -- take the reference's R[] from acorr_reference_kernel through the split scratch.
  a.certify = (q.flags & FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER) ? 0u : 1u;
  // REFERENCE_SUM_ORDER | INTEGER_PARITY_ONLY: the certified shapes keep their own order (launch_qlpc)
  a.integer_parity_only = ((q.flags & FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY) && (q.flags & FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER)) ? 1u : 0u;
  a.direct_mse = q.use_direct_mse ? 1u : 0u;  // (enqueue adds mae_steps and the scratch; elsewhere it keeps the launch off the fused wave kernel)
  return a;
}

void fixed_batch_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg) {
  a.lpc_order = 4;  // (no window, no quantisation: the fixed predictors)
  a.precision = 0;
  a.use_fixed = 1;
  a.fixed_max_order = cfg.fixed_max_order;
  a.fixed_order_sel = cfg.fixed_order_sel;
  a.fixed_partitions = cfg.fixed_partitions;
  if (cfg.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT) a.fixed_mode = 1;
}

void frame_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg, bool stereo, uint32_t group_log2) {
  a.use_constant = cfg.use_constant;
  a.use_lpc = cfg.use_lpc;
  a.use_leftside = stereo ? cfg.use_leftside : 0;
  a.use_rightside = stereo ? cfg.use_rightside : 0;
  a.use_midside = stereo ? cfg.use_midside : 0;
  a.use_fixed = cfg.use_fixed;
  a.fixed_max_order = cfg.fixed_max_order;
  a.fixed_order_sel = cfg.fixed_order_sel;
  a.fixed_group_log2 = group_log2;
}

void subwave_fields(QlpcKernelArgs& a, const flacenc_hip_frame_config& cfg, uint32_t cert_subwave) {
  a.stamps = nullptr;
  a.fixed_partitions = cfg.fixed_partitions;
  a.cert_subwave = cert_subwave;
}

ScratchGrant scratch_grant(const QlpcKernelArgs& a, LaunchKind kind, bool search) {
  const uint32_t n = a.block_size;
  const bool approx_ent = a.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT;
  switch (kind) {
    case LaunchKind::kLpcBatch:
      // R[] and the predictor records between the launches of the split pipelines: orders from 13, blocks of 8192 / 16384
      // at any order (the big-block kernels), the flagged orders, the estimators, the sub-wave kernel's clean-up counter
      // and, round 6, every unflagged launch: the reference's chains go in front of whatever kernel takes the shape
      return {a.lpc_order >= 13 || a.reference_order || a.direct_mse || n == 8192 || n == 16384 || subwave_shape(n) ||
              a.certify != 0u || search, false};
    case LaunchKind::kFixedBatch:
      // ApproxEnt: the big-block kernels' predictor records, the sub-wave kernel's clean-up counter; BitCount: neither
      return {approx_ent && (n == 4096 || n == 8192 || n == 16384 || subwave_shape(n)), approx_ent && a.reference_order != 0u};
    case LaunchKind::kFrame:
      // R[] of the reference-order pass: a flagged order, or a certified shape that cannot certify inside the fused
      // kernel (kReferencePass: off it, or with the bit writer, which is handed the reference's R[])
      return {a.reference_order != 0u ||
                  (a.certify != 0u && cert_shape(a) && !a.direct_mse && a.fixed_mode == 0 &&
                   (!wave_kernel_eligible(a) || a.pack_out != nullptr)),
              a.reference_order != 0u && a.use_fixed && approx_ent};
    case LaunchKind::kSubwaveFrames:
      return {true, false};  // the marked counters, and R[] under cert_subwave
  }
  return {false, false};
}

QlpcKernelArgs probe_record(const FrameCall& c, const FramePlan& p, LaunchKind kind) {
  QlpcKernelArgs a = config_record(p.cfg.qlpc, c.samples, c.stride, c.block_size, c.stereo ? 4 : 1, nullptr, c.bits_per_sample, c.stereo);
  if (kind == LaunchKind::kFrame) {
    a.residual = const_cast<int32_t*>(c.residual);
    a.residual_stride = c.residual_stride;
    frame_fields(a, p.cfg, c.stereo, p.group_log2);
    if (c.stereo) a.frame_results = reinterpret_cast<flacenc_hip_stereo_frame_result*>(uintptr_t{0xC0000000});
    else a.chan_results = reinterpret_cast<flacenc_hip_channel_result*>(uintptr_t{0xC4000000});
    if (p.fused_pack) a.pack_out = reinterpret_cast<uint8_t*>(uintptr_t{0xD0000000});
    return a;
  }
  a.residual = reinterpret_cast<int32_t*>(uintptr_t{0x40000000});  // handle scratch: aligned, padded
  a.residual_stride = padded_stride(a.block_size);
  if (kind == LaunchKind::kFixedBatch) fixed_batch_fields(a, p.cfg);
  if (scratch_grant(a, kind, lpc_search(p.cfg.qlpc.flags)).split) a.split_scratch = reinterpret_cast<void*>(uintptr_t{0x20000000});
  return a;
}

FramePlan plan_frame_call(const FrameCall& c) {
  FramePlan p{};
  p.cfg = c.cfg;
  p.cfg.qlpc.flags = search_flags(c.extra_windows, c.precision_floor, c.cfg.qlpc.flags, c.cfg.qlpc.quant_precision);
  if (c.block_size < FLACENC_HIP_MIN_BLOCK_SIZE) p.cfg.use_fixed = p.cfg.use_lpc = 0;
  const flacenc_hip_frame_config& cfg = p.cfg;
  // a search flag: the candidate batches + the deciding kernel for every shape (FUSED_PACK ignored); RICE_ESCAPE: the same,
  // whatever the candidates -- the pass sits between the batches and the decision
  p.search_or_escape = (lpc_search(cfg.qlpc.flags) && cfg.use_lpc) || (cfg.qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE);
  // fixed_group_log2: with the ApproxEnt selector the estimator's partitions must be whole groups of 64-sample lanes, 2^g
  // lanes each; composite: they are not (a partition count that is no power of two).  (verify_fixed: 1..=64 partitions.)
  bool composite = false;
  if (cfg.use_fixed && cfg.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT) {
    const uint32_t parts = cfg.fixed_partitions;
    composite = (parts & (parts - 1)) != 0;
    for (uint32_t lanes = composite ? 1u : 64u / parts; lanes > 1; lanes >>= 1) ++p.group_log2;
  }
  p.frame_record = c.stereo || !p.search_or_escape;  // (the stereo call builds it whatever the path)
  if (!p.search_or_escape) {
    QlpcKernelArgs a = probe_record(c, p, LaunchKind::kFrame);
    const bool fused = !composite && wave_kernel_eligible(a);
    // (FUSED_PACK asks for the one-kernel form, TWO_STAGE_PACK overrides it: api_frames.cpp has the measurement)
    p.fused_pack = fused && c.stereo && c.pack && c.block_size == 4096 && (cfg.qlpc.flags & FLACENC_HIP_FLAG_FUSED_PACK) &&
                   !(cfg.qlpc.flags & FLACENC_HIP_FLAG_TWO_STAGE_PACK);
    if (fused) {
      p.path = FramePlan::kFused;
    } else if (c.stereo && cfg.use_lpc && !cfg.qlpc.use_direct_mse && rows_aligned(a) && bigblock_eligible(probe_record(c, p, LaunchKind::kLpcBatch)) &&
               (!cfg.use_fixed || bigblock_fixed_eligible(probe_record(c, p, LaunchKind::kFixedBatch)))) {
      p.path = FramePlan::kBigBlock;
    } else if (c.block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && subwave_shape(c.block_size)) {
      p.subwave_scratch = true;
      // (the unflagged order on these shapes is the reference's: its chains for every QLPC candidate in front)
      p.cert_subwave = (a.certify != 0u && a.reference_order == 0u && !a.direct_mse && cfg.use_lpc && cfg.qlpc.lpc_order <= 12) ? 1u : 0u;
      subwave_fields(a, cfg, p.cert_subwave);
      a.marked_count = reinterpret_cast<uint32_t*>(uintptr_t{0x70000000});  // (kSubwaveFrames: always granted)
      a.marked_unit = c.stereo ? 4 : 1;
      if (c.stereo ? subwave_frame_eligible(a) : subwave_channels_eligible(a)) p.path = FramePlan::kSubwave;
    }
  }
  p.lpc_batch = p.path != FramePlan::kFused && cfg.use_lpc;
  p.fixed_batch = p.path != FramePlan::kFused && cfg.use_fixed;
  return p;
}

}  // namespace flacenc_hip
