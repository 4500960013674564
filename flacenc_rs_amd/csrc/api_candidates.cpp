// api_candidates.cpp -- the candidate batches (estimated_qlpc and fixed_lpc over a batch of subframes): argument checks,
// the launch record, the scratch the split pipelines need, the order mode of the certified shapes, and the two
// enqueue functions every frame-level call goes through.
#include <cstdint>

#include "api_internal.h"
#include "direct_mse.h"
#include "order_search.h"
#include "rice_escape.h"

namespace {  // (the two kernels of this unit, outside flacenc_hip: their names in a kernel trace stay what they were)

// launch_adaptive (see there).  One thread behind a launch that carried the counters: its verdict -- (sequence number, hard subframes, analysed subframes)
// in one 64-bit store to the pinned word -- and the counters cleared for the next one.
__global__ void cert_feedback_kernel(uint32_t* counters, unsigned long long* out, uint32_t seq) {
  const unsigned long long analysed = counters[0], hard = counters[1] + counters[2];
  counters[0] = counters[1] = counters[2] = 0u;
  *out = ((unsigned long long)(seq & 0xFFFu) << 52) | ((hard & 0x3FFFFFFull) << 26) | (analysed & 0x3FFFFFFull);
}

// OrderSel::BitCount (coding.rs:243-264): first minimum of the per-order keys
__global__ void bitcount_pick_kernel(const unsigned long long* keys, uint32_t n, uint32_t n_orders,
                                     uint8_t* orders, unsigned long long* best_keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long best = keys[i];
  uint32_t bk = 0;
  for (uint32_t k = 1; k < n_orders; ++k) {
    const unsigned long long v = keys[(size_t)k * n + i];
    if (v < best) {
      best = v;
      bk = k;
    }
  }
  orders[i] = (uint8_t)bk;
  if (best_keys) best_keys[i] = best;
}

}  // namespace

namespace flacenc_hip {

// FLACENC_HIP_FLAG_WINDOW_SEARCH with no extra window is exactly the call with the summation-order flag in its place
// (with FLACENC_HIP_FLAG_ORDER_SEARCH: the ORDER_SEARCH call; with FLACENC_HIP_FLAG_ORDER_GUESS: the ORDER_GUESS call),
// and so is FLACENC_HIP_FLAG_PRECISION_SEARCH with the handle's floor at or above the config's quant_precision.
// Callers of the flagged entry points run their config through this once, after flacenc_hip_verify_config.
uint32_t search_flags(const flacenc_hip_handle* h, uint32_t flags, uint32_t quant_precision) {
  const uint32_t dropped =
      (((flags & FLACENC_HIP_FLAG_WINDOW_SEARCH) && h->lpc_windows.empty()) ? FLACENC_HIP_FLAG_WINDOW_SEARCH : 0u) |
      (((flags & FLACENC_HIP_FLAG_PRECISION_SEARCH) && h->precision_floor >= quant_precision)
           ? FLACENC_HIP_FLAG_PRECISION_SEARCH : 0u);
  if (!dropped) return flags;
  flags &= ~dropped;
  if (lpc_search(flags)) return flags;
  flags &= ~(FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY);
  if (!(flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER)) flags |= FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER;
  return flags;
}

// The LPC candidate of a (normalised) config comes from the search over windows and orders (order_search.h): the frame
// -level calls then take the candidate batches and the stand-alone deciding kernels for every shape.
bool lpc_search(uint32_t flags) {
  return (flags & (FLACENC_HIP_FLAG_ORDER_SEARCH | FLACENC_HIP_FLAG_WINDOW_SEARCH | FLACENC_HIP_FLAG_ORDER_GUESS |
                   FLACENC_HIP_FLAG_PRECISION_SEARCH)) != 0;
}

int check_batch_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, const int32_t* samples,
                     size_t n_subframes, uint32_t block_size, size_t stride,
                     flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride,
                     uint32_t min_block) {
  if (!h || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  int rc = flacenc_hip_verify_config(cfg);
  if (rc != FLACENC_HIP_OK) {
    h->last_error = "config::Qlpc / config::Prc verification failed";
    return rc;
  }
  // (the frame-level calls pass min_block = 1: a stream's last block may be shorter than
  // MIN_BLOCK_SIZE_FOR_PREDICTION; encode_subframe then skips both predictors, coding.rs:396)
  if (block_size < min_block || block_size > FLACENC_HIP_MAX_BLOCK_SIZE) {
    h->last_error = "block_size must be in 64..=32767 (1..=32767 for the frame-level calls)";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (n_subframes == 0) return FLACENC_HIP_OK;
  if (!samples || !params || !residual || stride < block_size || residual_stride < block_size ||
      n_subframes > 0x7FFFFFFFull) {
    h->last_error = "null pointer, stride < block_size, or too many subframes";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  return FLACENC_HIP_OK;
}

namespace {
// check_batch_args for the candidate-level batches (flacenc_hip_qlpc_batch, _stereo_qlpc_batch, _fixed_lpc_batch and
// their async forms): their records have no field for wasted bits, so FLACENC_HIP_FLAG_WASTED_BITS is refused there
int check_candidate_batch_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, const int32_t* samples,
                               size_t n_subframes, uint32_t block_size, size_t stride,
                               flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride) {
  const int rc = check_batch_args(h, cfg, samples, n_subframes, block_size, stride, params, residual, residual_stride);
  if (rc != FLACENC_HIP_OK) return rc;
  if (cfg->flags & FLACENC_HIP_FLAG_WASTED_BITS) {
    h->last_error = "FLACENC_HIP_FLAG_WASTED_BITS is for the frame-level calls only";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  return FLACENC_HIP_OK;
}

// QlpcKernelArgs::reference_order: 0 = the kernels' canonical sums, 1 = the stable build's orders
// (FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER), 2 = the simd-nightly build's (FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER)
uint32_t sum_order_mode(uint32_t flags) {
  if (flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER) return 2u;
  return (flags & FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER) ? 1u : 0u;
}

// The unflagged order on the fused kernel's shapes is certified (QlpcKernelArgs::certify; launch_qlpc decides where it
// applies).  Launches that cannot run it inside the fused kernel -- unaligned rows, FLACENC_HIP_FLAG_GENERIC_KERNEL, the
// fused bit writer -- take the reference's R[] from acorr_reference_kernel through the split scratch.
void set_certify(flacenc_hip_handle* h, flacenc_hip::QlpcKernelArgs& a, uint32_t flags) {
  a.certify = (flags & FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER) ? 0u : 1u;
  // REFERENCE_SUM_ORDER | INTEGER_PARITY_ONLY: the certified shapes keep their own order (launch_qlpc)
  a.integer_parity_only = ((flags & FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY) && (flags & FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER)) ? 1u : 0u;
  a.cert_stats = h->cert_stats;
}
}  // namespace

bool certify_needs_scratch(const flacenc_hip::QlpcKernelArgs& a) {
  return a.certify != 0u && flacenc_hip::cert_shape(a) && (a.reference_order == 0u || a.integer_parity_only) &&
         !a.direct_mse && a.fixed_mode == 0 && (!flacenc_hip::wave_kernel_eligible(a) || a.pack_out != nullptr);
}

QlpcKernelArgs base_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, const WindowEntry* win,
                         const int32_t* samples, size_t stride, uint32_t block_size, size_t n_subframes,
                         const uint8_t* bps, uint32_t bps_uniform, bool stereo) {
  QlpcKernelArgs a;
  a.samples = samples;
  a.stride = stride;
  a.block_size = block_size;
  a.n_subframes = static_cast<uint32_t>(n_subframes);
  a.bps = bps;
  a.bps_uniform = bps_uniform;
  a.stereo = stereo ? 1u : 0u;
  if (win) {
    a.window = win->dev;
    a.window_lanes = win->dev_lanes;
    a.flat_lo = win->flat_lo;
    a.flat_hi = win->flat_hi;
  }
  a.lpc_order = q.lpc_order;
  a.precision = q.quant_precision;
  a.max_rice_parameter = q.max_rice_parameter;
  a.rice_finest_only = (q.flags & FLACENC_HIP_FLAG_FINEST_RICE_ORDER) ? 1u : 0u;
  a.force_generic = (q.flags & FLACENC_HIP_FLAG_GENERIC_KERNEL) ? 1u : 0u;
  a.reference_order = sum_order_mode(q.flags);
  set_certify(h, a, q.flags);
  a.direct_mse = q.use_direct_mse ? 1u : 0u;  // (enqueue adds mae_steps and the scratch; elsewhere it keeps the launch off the fused wave kernel)
  return a;
}

int lpc_scratch(flacenc_hip_handle* h, size_t n_rows, uint32_t block_size, bool with_minmax, LpcScratch* out) {
  int rc;
  if ((rc = ensure(h, h->d_cparams, n_rows * sizeof(flacenc_hip_subframe_params))) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_cresid, n_rows * padded_stride(block_size) * 4)) != FLACENC_HIP_OK) return rc;
  if (with_minmax && (rc = ensure(h, h->d_minmax, n_rows * 2 * sizeof(int32_t))) != FLACENC_HIP_OK) return rc;
  out->params = static_cast<flacenc_hip_subframe_params*>(h->d_cparams.ptr);
  out->rows = static_cast<int32_t*>(h->d_cresid.ptr);
  out->minmax = with_minmax ? static_cast<int32_t*>(h->d_minmax.ptr) : nullptr;
  return FLACENC_HIP_OK;
}

int fixed_scratch(flacenc_hip_handle* h, size_t n_rows, uint32_t block_size, FixedScratch* out) {
  int rc;
  if ((rc = ensure(h, h->d_fparams, n_rows * sizeof(flacenc_hip_subframe_params))) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_fresid, n_rows * padded_stride(block_size) * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_fkeys, n_rows * 8)) != FLACENC_HIP_OK) return rc;
  out->params = static_cast<flacenc_hip_subframe_params*>(h->d_fparams.ptr);
  out->rows = static_cast<int32_t*>(h->d_fresid.ptr);
  out->keys = static_cast<unsigned long long*>(h->d_fkeys.ptr);
  return FLACENC_HIP_OK;
}

// FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER with the ApproxEnt selector: room for sumabs_reference_kernel's
// per-partition f32 sums (launch_qlpc runs it when `sumabs_scratch` is set)
int attach_sumabs_scratch(flacenc_hip_handle* h, flacenc_hip::QlpcKernelArgs& a, bool approx_ent) {
  if (!a.reference_order || !approx_ent) return FLACENC_HIP_OK;
  int rc = ensure(h, h->d_sumabs, static_cast<size_t>(a.n_subframes) * 5 * 64 * sizeof(float));
  if (rc != FLACENC_HIP_OK) return rc;
  a.sumabs_scratch = static_cast<float*>(h->d_sumabs.ptr);
  return FLACENC_HIP_OK;
}

// R[] and the predictor records between the launches of the split pipelines, and the counter through which
// bigblock_residual_kernel tells the clean-up launch whether it marked anything (QlpcKernelArgs::marked_count).
// The pipeline's own counter is cleared on its stream here: a pipeline that attached this scratch but had no clean-up
// launch behind it (the fused 4096 / 4608 kernels, for one) leaves its count and list entries in the other slot, and
// the pipeline after the next one would otherwise start from them and visit records twice.
int attach_split_scratch(flacenc_hip_handle* h, flacenc_hip::QlpcKernelArgs& a, void* stream) {
  int rc = ensure(h, h->d_split, static_cast<size_t>(a.n_subframes) * (33 * 8 + 36 * 4));
  if (rc != FLACENC_HIP_OK) return rc;
  a.split_scratch = h->d_split.ptr;
  // two counters (16 words reserved) + a list of the first kMarkedCap marks behind each
  constexpr uint32_t kMarkedCap = 1024;
  constexpr size_t kMarkedBytes = 64 + 2 * static_cast<size_t>(kMarkedCap) * 4;
  if (h->d_marked.ptr == nullptr) {
    if ((rc = ensure(h, h->d_marked, kMarkedBytes)) != FLACENC_HIP_OK) return rc;
    HIP_TRY(h, hipMemset(h->d_marked.ptr, 0, kMarkedBytes));
  }
  h->marked_parity ^= 1u;
  a.marked_count = static_cast<uint32_t*>(h->d_marked.ptr) + h->marked_parity;
  a.marked_next = static_cast<uint32_t*>(h->d_marked.ptr) + (h->marked_parity ^ 1u);
  a.marked_list = static_cast<uint32_t*>(h->d_marked.ptr) + 16 + h->marked_parity * kMarkedCap;
  a.marked_cap = kMarkedCap;
  a.marked_unit = 1;
  HIP_TRY(h, hipMemsetAsync(a.marked_count, 0, 4, static_cast<hipStream_t>(stream)));
  return FLACENC_HIP_OK;
}

namespace {
// The certified shapes (blocks of 4096 / 4608 samples at orders up to 12) by material.  The fused kernel settles a
// subframe's order certificate in its first tier for next to nothing; the second tier and the recomputation from the
// reference's chains are serial work of one wave while its workgroup waits -- rare on noise-like material (2 subframes in
// 393 216 of the bench signal), the rule on music (the reference's real-audio fixtures: 26 % / 82 % / 100 % of the
// subframes at orders 8 / 10 / 12 count as unsettled, 220 / 146 / 100 G samples/s where the bench signal runs at 350).  Two passes -- the
// reference's chains on the matrix cores for every subframe, then the fused kernel on their R[] -- give the SAME integers
// at a flat 1.4 x the certified kernel's best time.  So launches that return integers only (no R[], no coefficients: their
// bits depend on the pass that produced them) watch the certificate's counters and take the two-pass form while the
// material they were last given was hard: above kHardShare of the subframes unsettled by the first tier, for a span of
// launches that doubles (8 .. 64) while the probes between the spans keep finding it so.
constexpr double kHardShare = 0.10;
// a verdict is taken from at least this many subframes (counters of smaller launches add up until they are), a probe's from
// at least kProbeMinSubframes; launches of 2^25 subframes and more are not watched (the verdict's fields are 26 bits wide)
constexpr uint32_t kFeedbackMinSubframes = 4096, kProbeMinSubframes = 1024, kFeedbackMaxSubframes = 1u << 25;
inline uint32_t next_seq(uint32_t seq) { return ((seq + 1u) & 0xFFFu) ? ((seq + 1u) & 0xFFFu) : 1u; }  // (0: the word's initial state)
}  // namespace

int launch_adaptive(flacenc_hip_handle* h, flacenc_hip::QlpcKernelArgs& a, const flacenc_hip::QlpcLaunchPlan& plan,
                    hipStream_t stream) {
  const bool fused_certified = flacenc_hip::plan_qlpc_route(a).order == flacenc_hip::QlpcRoute::kCertifiedFused;
  const bool watch = fused_certified && h->adaptive_order != 0 && h->cert_stats == nullptr && a.autocorr == nullptr &&
                     a.lpc_coefs == nullptr && a.n_subframes < kFeedbackMaxSubframes;
  if (!watch) {
    HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
    return FLACENC_HIP_OK;
  }
  if (h->d_cert_fb == nullptr) {
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_cert_fb), 16));
    HIP_TRY(h, hipMemset(h->d_cert_fb, 0, 16));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_cert_fb), 8, hipHostMallocMapped));
    *h->h_cert_fb = 0ull;
  }
  // The latest verdict that has landed (a plain read of the pinned word: late is fine, torn it cannot be).  The host may
  // run many launches ahead of the device, so nothing is concluded from launches whose counters are not in: on easy
  // material every launch carries the counters and any new verdict counts; on hard material a span of two-pass launches
  // is followed by ONE probe (a certified launch), and the launches behind the probe stay two-pass until ITS verdict is in.
  const unsigned long long word = *reinterpret_cast<volatile unsigned long long*>(h->h_cert_fb);
  const uint32_t l_seq = static_cast<uint32_t>(word >> 52), l_hard = static_cast<uint32_t>(word >> 26) & 0x3FFFFFFu,
                 l_an = static_cast<uint32_t>(word) & 0x3FFFFFFu;
  const bool is_hard = l_an != 0u && static_cast<double>(l_hard) > kHardShare * static_cast<double>(l_an);
  bool two_pass;
  if (h->two_pass_span == 0) {  // easy so far
    if (l_seq != h->fb_seen_seq) {
      h->fb_seen_seq = l_seq;
      if (is_hard) h->two_pass_left = h->two_pass_span = 8;
    }
    two_pass = h->two_pass_span != 0;
  } else if (h->two_pass_left > 0) {
    two_pass = true;
  } else if (!h->fb_probe_out) {
    two_pass = false;  // the probe: certified launches until kProbeMinSubframes have been counted
    h->fb_probe_out = true;
    h->fb_probe_seq = 0u;  // (assigned when its feedback goes out)
  } else if (h->fb_probe_seq == 0u) {
    two_pass = false;  // the probe is still collecting
  } else if (l_seq != h->fb_probe_seq) {
    two_pass = true;  // the probe's verdict is not in yet
  } else {
    h->fb_probe_out = false;
    h->fb_seen_seq = l_seq;
    if (is_hard) {
      h->two_pass_span = h->two_pass_span >= 64 ? 64 : 2 * h->two_pass_span;
      h->two_pass_left = h->two_pass_span;
      two_pass = true;
    } else {
      h->two_pass_span = 0;
      two_pass = false;
    }
  }
  if (two_pass) {
    if (h->two_pass_left > 0) --h->two_pass_left;
    flacenc_hip::QlpcKernelArgs b = a;
    b.certify = 0;
    b.reference_order = 1u;  // (the autocorrelation alone: the selector's sums follow sumabs_scratch, which the flags decide)
    if (b.split_scratch == nullptr) {
      int rc = attach_split_scratch(h, b, stream);
      if (rc != FLACENC_HIP_OK) return rc;
    }
    HIP_TRY(h, flacenc_hip::launch_qlpc(b, plan, stream));
    return FLACENC_HIP_OK;
  }
  a.cert_stats = h->d_cert_fb;
  HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
  h->fb_pending += a.n_subframes;
  const bool probing = h->fb_probe_out && h->fb_probe_seq == 0u;
  if (h->fb_pending >= (probing ? kProbeMinSubframes : kFeedbackMinSubframes)) {
    h->fb_pending = 0;
    h->fb_seq = next_seq(h->fb_seq);
    if (probing) h->fb_probe_seq = h->fb_seq;
    unsigned long long* out = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&out), h->h_cert_fb, 0));
    hipLaunchKernelGGL(cert_feedback_kernel, dim3(1), dim3(1), 0, stream, h->d_cert_fb, out, h->fb_seq);
    HIP_TRY(h, hipGetLastError());
  }
  return FLACENC_HIP_OK;
}

// FLACENC_HIP_FLAG_RICE_ESCAPE: the post-pass over the records and rows a candidate batch has just enqueued
// (rice_escape.cpp)
int enqueue_rice_escape(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, flacenc_hip_subframe_params* params,
                        const int32_t* residual, size_t residual_stride, size_t n_subframes, uint32_t block_size,
                        hipStream_t stream) {
  flacenc_hip::RiceEscapeArgs e{};
  e.params = params;
  e.residual = residual;
  e.residual_stride = residual_stride;
  e.block_size = block_size;
  e.n_rows = static_cast<uint32_t>(n_subframes);
  e.max_rice_parameter = q.max_rice_parameter;
  e.finest_only = (q.flags & FLACENC_HIP_FLAG_FINEST_RICE_ORDER) ? 1u : 0u;
  HIP_TRY(h, flacenc_hip::launch_rice_escape(e, stream));
  return FLACENC_HIP_OK;
}

namespace {
int enqueue_lpc(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, const int32_t* samples,
                size_t n_subframes, uint32_t block_size, size_t stride, const uint8_t* bps,
                flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride,
                double* autocorr, double* lpc_coefs, hipStream_t stream, bool stereo, uint32_t bps_uniform,
                int32_t* residual_lr, size_t residual_lr_stride, int32_t* minmax_out, bool* placed,
                uint32_t residual_mode) {
  if (placed) *placed = false;
  flacenc_hip_qlpc_config qcfg = *cfg;
  qcfg.flags = search_flags(h, cfg->flags, cfg->quant_precision);
  cfg = &qcfg;
  const WindowEntry* win = nullptr;
  int rc = get_window(h, cfg, block_size, &win);
  if (rc != FLACENC_HIP_OK) return rc;
  const float* const win_dev = win->dev;  // (get_window_entry may grow h->windows below)
  flacenc_hip::QlpcLaunchPlan plan = flacenc_hip::plan_qlpc_launch(block_size, cfg->lpc_order);
  if (plan.smem_bytes > 160 * 1024) {
    h->last_error = "internal: LDS plan exceeds 160 KiB";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  QlpcKernelArgs a = base_args(h, *cfg, win, samples, stride, block_size, n_subframes, bps, bps_uniform, stereo);
  a.params = params;
  a.residual = residual;
  a.residual_stride = residual_stride;
  a.autocorr = autocorr;
  a.lpc_coefs = lpc_coefs;
  a.stamps = h->stamps;
  a.mae_steps = cfg->use_direct_mse ? cfg->mae_optimization_steps : 0u;  // (ignored without it, coding.rs:337-347)
  if (a.direct_mse && flacenc_hip::direct_mse_lds_bytes(block_size, a.mae_steps > 0, cfg->lpc_order) > 160 * 1024) {
    h->last_error = "use_direct_mse: the block does not fit the LDS";  // (not for any block up to 32767 samples)
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  if (a.direct_mse) {
    // (R[] and the matrix between the chains and the lane-per-subframe solve; with IRLS steps also the iteration's state)
    rc = ensure(h, h->d_gram, n_subframes * (flacenc_hip::direct_mse_gram_stride(cfg->lpc_order) +
                                             (a.mae_steps ? flacenc_hip::kIrlsStateDoubles : 0)) * sizeof(double));
    if (rc != FLACENC_HIP_OK) return rc;
    a.direct_mse_scratch = static_cast<double*>(h->d_gram.ptr);
  }
  if (a.direct_mse && a.mae_steps > 0) {
    // the IRLS weights between the steps' kernels (orders up to 11); lpc_with_irls_mae (lpc.rs:814-850) has no block
    // limit: above 16384 samples the one-kernel form keeps them here too
    rc = ensure(h, h->d_irlsw, n_subframes * padded_stride(block_size) * sizeof(float));
    if (rc != FLACENC_HIP_OK) return rc;
    a.irls_weight_scratch = static_cast<float*>(h->d_irlsw.ptr);
  }
  // (R[] and the predictor records between the launches of the split pipelines: orders from 13, and blocks of
  // 8192 / 16384 at any order -- the big-block kernels)
  // (... and, round 6, every unflagged launch: the reference's chains go in front of whatever kernel takes the shape)
  const bool order_search = lpc_search(cfg->flags);
  if (cfg->lpc_order >= 13 || a.reference_order || a.direct_mse || block_size == 8192 || block_size == 16384 ||
      flacenc_hip::subwave_shape(block_size) || a.certify != 0u || order_search) {
    if ((rc = attach_split_scratch(h, a, stream)) != FLACENC_HIP_OK) return rc;
  }
  if (plan.table_scratch_bytes_per_subframe) {
    rc = ensure(h, h->d_tables, plan.table_scratch_bytes_per_subframe * n_subframes);
    if (rc != FLACENC_HIP_OK) return rc;
    a.table_scratch = static_cast<uint32_t*>(h->d_tables.ptr);
  }
  if (order_search) {
    // FLACENC_HIP_FLAG_ORDER_SEARCH / _WINDOW_SEARCH / _ORDER_GUESS / _PRECISION_SEARCH (DESIGN.md 4.10, 4.11, 4.13,
    // 4.16): R[] of every window in the stable build's order (nightly's with its flag; the certificate and
    // INTEGER_PARITY_ONLY do not apply), every candidate (window, order, precision) searched -- under ORDER_GUESS (0, P)
    // and every window's K guesses, K as the handle holds it now; under PRECISION_SEARCH every precision from
    // quant_precision down to the handle's floor as it is now (search_flags: below quant_precision) --, the records
    // written by stage 3
    a.certify = 0;
    a.integer_parity_only = 0;
    a.cert_stats = nullptr;
    flacenc_hip::SearchShape shape{};
    shape.windows[0] = win_dev;
    shape.n_windows = 1;
    shape.guess_orders = (cfg->flags & FLACENC_HIP_FLAG_ORDER_GUESS) ? h->order_guesses : 0u;
    shape.search_orders = ((cfg->flags & FLACENC_HIP_FLAG_ORDER_SEARCH) || shape.guess_orders) ? 1u : 0u;
    shape.guess_trace = shape.guess_orders ? h->order_guess_trace : nullptr;
    shape.n_precisions =
        (cfg->flags & FLACENC_HIP_FLAG_PRECISION_SEARCH) ? cfg->quant_precision - h->precision_floor + 1u : 1u;
    if (cfg->flags & FLACENC_HIP_FLAG_WINDOW_SEARCH) {
      for (const LpcWindow& w : h->lpc_windows) {
        const WindowEntry* e = nullptr;
        if ((rc = get_window_entry(h, w.type, w.alpha, w.start, w.end, block_size, &e)) != FLACENC_HIP_OK) return rc;
        shape.windows[shape.n_windows++] = e->dev;
      }
    }
    rc = ensure(h, h->d_order, flacenc_hip::order_search_scratch_bytes(a.n_subframes, cfg->lpc_order, shape));
    if (rc != FLACENC_HIP_OK) return rc;
    HIP_TRY(h, flacenc_hip::launch_order_search(a, plan, a.reference_order == 2u ? 1u : 0u, shape, h->d_order.ptr,
                                                stream, &h->last_search_slices));
    return FLACENC_HIP_OK;
  }
  // frame-level callers on the big-block shapes: L / R candidates straight into the output rows, role min / max
  // from the residual kernel (only bigblock_residual_kernel knows how; see QlpcKernelArgs::residual_lr)
  if (stereo && residual_lr != nullptr && minmax_out != nullptr &&
      (reinterpret_cast<uintptr_t>(residual_lr) & 15) == 0 && (residual_lr_stride & 3) == 0 &&
      (flacenc_hip::bigblock_eligible(a) || (a.direct_mse && flacenc_hip::bigblock_shape_eligible(a)))) {
    a.residual_lr = residual_lr;
    a.residual_lr_stride = residual_lr_stride;
    a.minmax_out = minmax_out;
    if (placed) *placed = true;
  }
  // ... or, with residual_mode 1, no rows at all: records and the roles' min / max only (the deciding store pass,
  // bigblock_residual_kernel's mode 2, produces the two rows the frame keeps)
  if (stereo && residual_mode == 1u && minmax_out != nullptr &&
      (flacenc_hip::bigblock_eligible(a) || (a.direct_mse && flacenc_hip::bigblock_shape_eligible(a)))) {
    a.residual_mode = 1u;
    a.minmax_out = minmax_out;
    if (placed) *placed = true;
  }
  return launch_adaptive(h, a, plan, stream);
}
}  // namespace

// The one exit of the LPC candidates.  Under FLACENC_HIP_FLAG_RICE_ESCAPE every record and row goes to `params` /
// `residual` (no rows placed in the caller's frame, no analyse-only launch) and the escape pass runs behind them -- on
// the winner's record where a search flag chose one.
int enqueue(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, const int32_t* samples,
            size_t n_subframes, uint32_t block_size, size_t stride, const uint8_t* bps,
            flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride,
            double* autocorr, double* lpc_coefs, hipStream_t stream, bool stereo, uint32_t bps_uniform,
            int32_t* residual_lr, size_t residual_lr_stride, int32_t* minmax_out, bool* placed,
            uint32_t residual_mode) {
  if (!(cfg->flags & FLACENC_HIP_FLAG_RICE_ESCAPE))
    return enqueue_lpc(h, cfg, samples, n_subframes, block_size, stride, bps, params, residual, residual_stride, autocorr,
                       lpc_coefs, stream, stereo, bps_uniform, residual_lr, residual_lr_stride, minmax_out, placed,
                       residual_mode);
  if (residual_mode != 0u) {
    h->last_error = "internal: analyse-only QLPC batch under FLACENC_HIP_FLAG_RICE_ESCAPE";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  int rc = enqueue_lpc(h, cfg, samples, n_subframes, block_size, stride, bps, params, residual, residual_stride, autocorr,
                       lpc_coefs, stream, stereo, bps_uniform, nullptr, 0, nullptr, placed, 0u);
  if (rc != FLACENC_HIP_OK) return rc;
  return enqueue_rice_escape(h, *cfg, params, residual, residual_stride, n_subframes, block_size, stream);
}

// config::Fixed::verify (config.rs:246-255) + OrderSel::verify (:419-431)
int verify_fixed(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg) {
  if (cfg->fixed_max_order > FLACENC_HIP_MAX_FIXED_LPC_ORDER ||
      (cfg->fixed_order_sel != FLACENC_HIP_ORDERSEL_BITCOUNT &&
       cfg->fixed_order_sel != FLACENC_HIP_ORDERSEL_APPROXENT) ||
      (cfg->fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT &&
       (cfg->fixed_partitions < 1 || cfg->fixed_partitions > 64))) {
    h->last_error = "fixed: max_order must be ..=4, order_sel BitCount / ApproxEnt, ApproxEnt.partitions 1..=64";
    return FLACENC_HIP_ERR_BAD_CONFIG;
  }
  return FLACENC_HIP_OK;
}

// `fixed_lpc` (coding.rs:298-331) for a batch, device pointers, on `stream`
int enqueue_fixed(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* samples,
                  size_t n_subframes, uint32_t block_size, size_t stride, const uint8_t* bps,
                  uint32_t bps_uniform, bool stereo, flacenc_hip_subframe_params* params, int32_t* residual,
                  size_t residual_stride, unsigned long long* selector_keys, hipStream_t stream,
                  uint32_t residual_mode) {
  int rc = verify_fixed(h, cfg);
  if (rc != FLACENC_HIP_OK) return rc;
  // FLACENC_HIP_FLAG_RICE_ESCAPE: the pass runs on the selected order's record; the selector's keys (and BitCount's
  // comparison of unescaped code_bits) are what they are without the flag
  auto escape = [&](int done) -> int {
    if (done != FLACENC_HIP_OK || !(cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE)) return done;
    return enqueue_rice_escape(h, cfg->qlpc, params, residual, residual_stride, n_subframes, block_size, stream);
  };
  if ((cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE) && residual_mode != 0u) {
    h->last_error = "internal: analyse-only fixed_lpc batch under FLACENC_HIP_FLAG_RICE_ESCAPE";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  flacenc_hip::QlpcLaunchPlan plan = flacenc_hip::plan_qlpc_launch(block_size, 4);
  if (plan.smem_bytes > 160 * 1024) {
    h->last_error = "internal: LDS plan exceeds 160 KiB";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  QlpcKernelArgs a = base_args(h, cfg->qlpc, nullptr, samples, stride, block_size, n_subframes, bps, bps_uniform, stereo);
  a.lpc_order = 4;  // (no window, no quantisation: the fixed predictors)
  a.precision = 0;
  a.params = params;
  a.residual = residual;
  a.residual_stride = residual_stride;
  a.use_fixed = 1;
  a.fixed_max_order = cfg->fixed_max_order;
  a.fixed_order_sel = cfg->fixed_order_sel;
  a.fixed_keys = h->fixed_keys;
  a.fixed_partitions = cfg->fixed_partitions;
  a.selector_keys = selector_keys;
  if (plan.table_scratch_bytes_per_subframe) {
    rc = ensure(h, h->d_tables, plan.table_scratch_bytes_per_subframe * n_subframes);
    if (rc != FLACENC_HIP_OK) return rc;
    a.table_scratch = static_cast<uint32_t*>(h->d_tables.ptr);
  }
  if (cfg->fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT) {
    a.fixed_mode = 1;
    if ((rc = attach_sumabs_scratch(h, a, true)) != FLACENC_HIP_OK) return rc;
    if (block_size == 4096 || block_size == 8192 || block_size == 16384 ||  // the big-block kernels' predictor records
        flacenc_hip::subwave_shape(block_size)) {                            // ... the sub-wave kernel's clean-up counter
      if ((rc = attach_split_scratch(h, a, stream)) != FLACENC_HIP_OK) return rc;
    }
    if (residual_mode == 1u) {  // (the caller checked that this launch takes the big-block kernels)
      if (!flacenc_hip::bigblock_fixed_eligible(a)) {
        h->last_error = "internal: analyse-only fixed_lpc batch on a shape the big-block kernels do not take";
        return FLACENC_HIP_ERR_UNSUPPORTED;
      }
      a.residual_mode = 1u;
    }
    HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
    return escape(FLACENC_HIP_OK);
  }
  // BitCount: code every order, keep the first minimum of bps*order + code_bits, code it again
  const uint32_t n_orders = cfg->fixed_max_order + 1;
  if ((rc = ensure(h, h->d_keys, n_subframes * n_orders * 8)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_sel, n_subframes)) != FLACENC_HIP_OK) return rc;
  unsigned long long* keys = static_cast<unsigned long long*>(h->d_keys.ptr);
  for (uint32_t k = 0; k < n_orders; ++k) {
    a.fixed_mode = 2;
    a.forced_uniform = k;
    a.selector_keys = keys + static_cast<size_t>(k) * n_subframes;
    HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
    if (h->fixed_keys) {  // test hook: keys[sf*8 + k]
      HIP_TRY(h, hipMemcpy2DAsync(h->fixed_keys + k, 8 * 8, a.selector_keys, 8, 8, n_subframes,
                                  hipMemcpyDeviceToDevice, stream));
    }
  }
  const uint32_t n32 = static_cast<uint32_t>(n_subframes);
  hipLaunchKernelGGL(bitcount_pick_kernel, dim3((n32 + 255) / 256), dim3(256), 0, stream, keys, n32, n_orders,
                     static_cast<uint8_t*>(h->d_sel.ptr), selector_keys);
  HIP_TRY(h, hipGetLastError());
  a.fixed_mode = 3;
  a.forced_orders = static_cast<const uint8_t*>(h->d_sel.ptr);
  a.selector_keys = nullptr;
  HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
  return escape(FLACENC_HIP_OK);
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" {

int flacenc_hip_qlpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                 const int32_t* samples, size_t n_subframes, uint32_t block_size,
                                 size_t stride, const uint8_t* bps,
                                 flacenc_hip_subframe_params* params, int32_t* residual,
                                 size_t residual_stride, double* autocorr, double* lpc_coefs,
                                 void* stream) {
  int rc = check_candidate_batch_args(h, cfg, samples, n_subframes, block_size, stride, params, residual,
                                      residual_stride);
  if (rc != FLACENC_HIP_OK || n_subframes == 0) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = HIP's default (null) stream
  return enqueue(h, cfg, samples, n_subframes, block_size, stride, bps, params, residual,
                 residual_stride, autocorr, lpc_coefs, s);
}

int flacenc_hip_qlpc_batch(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                           const int32_t* samples, size_t n_subframes, uint32_t block_size,
                           size_t stride, const uint8_t* bps,
                           flacenc_hip_subframe_params* params, int32_t* residual,
                           size_t residual_stride, double* autocorr, double* lpc_coefs,
                           int memory_kind) {
  int rc = check_candidate_batch_args(h, cfg, samples, n_subframes, block_size, stride, params, residual,
                                      residual_stride);
  if (rc != FLACENC_HIP_OK || n_subframes == 0) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, enqueue(h, cfg, samples, n_subframes, block_size, stride, bps, params, residual, residual_stride,
                              autocorr, lpc_coefs, h->stream), false);
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  // host pointers: stage through the handle's device scratch (PCIe both ways)
  const size_t dstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_samples, n_subframes * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_subframes * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_params, n_subframes * sizeof(flacenc_hip_subframe_params))) != FLACENC_HIP_OK)
    return rc;
  if (bps && (rc = ensure(h, h->d_bps, n_subframes)) != FLACENC_HIP_OK) return rc;
  if (autocorr && (rc = ensure(h, h->d_autocorr, n_subframes * 33 * 8)) != FLACENC_HIP_OK) return rc;
  if (lpc_coefs && (rc = ensure(h, h->d_lpc, n_subframes * 32 * 8)) != FLACENC_HIP_OK) return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, samples, stride, block_size, n_subframes)) != FLACENC_HIP_OK) return rc;
  if (bps) HIP_TRY(h, hipMemcpyAsync(h->d_bps.ptr, bps, n_subframes, hipMemcpyHostToDevice, s));
  rc = enqueue(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), n_subframes, block_size, dstride,
               bps ? static_cast<const uint8_t*>(h->d_bps.ptr) : nullptr,
               static_cast<flacenc_hip_subframe_params*>(h->d_params.ptr),
               static_cast<int32_t*>(h->d_residual.ptr), dstride,
               autocorr ? static_cast<double*>(h->d_autocorr.ptr) : nullptr,
               lpc_coefs ? static_cast<double*>(h->d_lpc.ptr) : nullptr, s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, residual, residual_stride, h->d_residual, block_size, n_subframes)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(params, h->d_params.ptr, n_subframes * sizeof(flacenc_hip_subframe_params),
                            hipMemcpyDeviceToHost, s));
  if (autocorr)
    HIP_TRY(h, hipMemcpyAsync(autocorr, h->d_autocorr.ptr, n_subframes * 33 * 8, hipMemcpyDeviceToHost, s));
  if (lpc_coefs)
    HIP_TRY(h, hipMemcpyAsync(lpc_coefs, h->d_lpc.ptr, n_subframes * 32 * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_stereo_qlpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                        const int32_t* frames, size_t n_frames, uint32_t block_size,
                                        size_t stride, uint32_t bits_per_sample,
                                        flacenc_hip_subframe_params* params, int32_t* residual,
                                        size_t residual_stride, void* stream) {
  int rc = check_candidate_batch_args(h, cfg, frames, n_frames * 4, block_size, stride, params, residual,
                                      residual_stride);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  if (bits_per_sample < 8 || bits_per_sample > 24) {
    h->last_error = "bits_per_sample must be in 8..=24";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = HIP's default (null) stream
  return enqueue(h, cfg, frames, n_frames * 4, block_size, stride, nullptr, params, residual,
                 residual_stride, nullptr, nullptr, s, true, bits_per_sample);
}

int flacenc_hip_stereo_qlpc_batch(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                  const int32_t* frames, size_t n_frames, uint32_t block_size,
                                  size_t stride, uint32_t bits_per_sample,
                                  flacenc_hip_subframe_params* params, int32_t* residual,
                                  size_t residual_stride, int memory_kind) {
  if (memory_kind == FLACENC_HIP_MEM_DEVICE) {
    if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
    return drained(h, flacenc_hip_stereo_qlpc_batch_async(h, cfg, frames, n_frames, block_size, stride, bits_per_sample,
                                                          params, residual, residual_stride, h->stream), n_frames == 0);
  }
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  int rc = check_candidate_batch_args(h, cfg, frames, n_frames * 4, block_size, stride, params, residual,
                                      residual_stride);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t dstride = padded_stride(block_size);
  const size_t n_sub = n_frames * 4;
  if ((rc = ensure(h, h->d_samples, n_frames * 2 * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_sub * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_params, n_sub * sizeof(flacenc_hip_subframe_params))) != FLACENC_HIP_OK)
    return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, frames, stride, block_size, n_frames * 2)) != FLACENC_HIP_OK) return rc;
  rc = flacenc_hip_stereo_qlpc_batch_async(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr),
                                           n_frames, block_size, dstride, bits_per_sample,
                                           static_cast<flacenc_hip_subframe_params*>(h->d_params.ptr),
                                           static_cast<int32_t*>(h->d_residual.ptr), dstride, s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, residual, residual_stride, h->d_residual, block_size, n_sub)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(params, h->d_params.ptr, n_sub * sizeof(flacenc_hip_subframe_params),
                            hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_fixed_lpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                      const int32_t* samples, size_t n_units, uint32_t block_size,
                                      size_t stride, const uint8_t* bps, uint32_t bits_per_sample, int layout,
                                      flacenc_hip_subframe_params* params, int32_t* residual,
                                      size_t residual_stride, uint64_t* selector_keys, void* stream) {
  if (!h || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const bool stereo = layout == FLACENC_HIP_LAYOUT_STEREO_FRAMES;
  if (!stereo && layout != FLACENC_HIP_LAYOUT_SUBFRAMES) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const size_t n_sub = stereo ? n_units * 4 : n_units;
  int rc = check_candidate_batch_args(h, &cfg->qlpc, samples, n_sub, block_size, stride, params, residual, residual_stride);
  if (rc != FLACENC_HIP_OK || n_units == 0) return rc;
  if (!bps && (bits_per_sample < 8 || bits_per_sample > 25)) {
    h->last_error = "bits_per_sample must be in 8..=25 when no per-subframe bps array is given";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  return enqueue_fixed(h, cfg, samples, n_sub, block_size, stride, stereo ? nullptr : bps, bits_per_sample, stereo,
                       params, residual, residual_stride, reinterpret_cast<unsigned long long*>(selector_keys),
                       static_cast<hipStream_t>(stream));
}

int flacenc_hip_fixed_lpc_batch(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                const int32_t* samples, size_t n_units, uint32_t block_size, size_t stride,
                                const uint8_t* bps, uint32_t bits_per_sample, int layout,
                                flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride,
                                uint64_t* selector_keys, int memory_kind) {
  if (!h || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, flacenc_hip_fixed_lpc_batch_async(h, cfg, samples, n_units, block_size, stride, bps, bits_per_sample,
                                                        layout, params, residual, residual_stride, selector_keys, h->stream),
                   n_units == 0);
  if (memory_kind != FLACENC_HIP_MEM_HOST) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const bool stereo = layout == FLACENC_HIP_LAYOUT_STEREO_FRAMES;
  if (!stereo && layout != FLACENC_HIP_LAYOUT_SUBFRAMES) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const size_t n_sub = stereo ? n_units * 4 : n_units;
  const size_t n_rows = stereo ? n_units * 2 : n_units;
  int rc = check_candidate_batch_args(h, &cfg->qlpc, samples, n_sub, block_size, stride, params, residual, residual_stride);
  if (rc != FLACENC_HIP_OK || n_units == 0) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t dstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_samples, n_rows * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_sub * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_params, n_sub * sizeof(flacenc_hip_subframe_params))) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_autocorr, n_sub * 8)) != FLACENC_HIP_OK) return rc;  // selector keys
  if (bps && !stereo && (rc = ensure(h, h->d_bps, n_sub)) != FLACENC_HIP_OK) return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, samples, stride, block_size, n_rows)) != FLACENC_HIP_OK) return rc;
  if (bps && !stereo) HIP_TRY(h, hipMemcpyAsync(h->d_bps.ptr, bps, n_sub, hipMemcpyHostToDevice, s));
  rc = flacenc_hip_fixed_lpc_batch_async(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), n_units, block_size,
                                         dstride, (bps && !stereo) ? static_cast<const uint8_t*>(h->d_bps.ptr) : nullptr,
                                         bits_per_sample, layout,
                                         static_cast<flacenc_hip_subframe_params*>(h->d_params.ptr),
                                         static_cast<int32_t*>(h->d_residual.ptr), dstride,
                                         static_cast<uint64_t*>(h->d_autocorr.ptr), s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, residual, residual_stride, h->d_residual, block_size, n_sub)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(params, h->d_params.ptr, n_sub * sizeof(flacenc_hip_subframe_params),
                            hipMemcpyDeviceToHost, s));
  if (selector_keys)
    HIP_TRY(h, hipMemcpyAsync(selector_keys, h->d_autocorr.ptr, n_sub * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

}  // extern "C"
