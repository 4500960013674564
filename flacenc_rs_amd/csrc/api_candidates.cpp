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

int check_bits_per_sample(flacenc_hip_handle* h, uint32_t bits_per_sample) {
  if (bits_per_sample >= 8 && bits_per_sample <= 24) return FLACENC_HIP_OK;
  h->last_error = "bits_per_sample must be in 8..=24";
  return FLACENC_HIP_ERR_BAD_ARGUMENT;
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
}  // namespace

QlpcKernelArgs base_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, const WindowEntry* win,
                         const int32_t* samples, size_t stride, uint32_t block_size, size_t n_subframes,
                         const uint8_t* bps, uint32_t bps_uniform, bool stereo) {
  QlpcKernelArgs a = config_record(q, samples, stride, block_size, n_subframes, bps, bps_uniform, stereo);
  if (win) {
    a.window = win->dev;
    a.window_lanes = win->dev_lanes;
    a.flat_lo = win->flat_lo;
    a.flat_hi = win->flat_hi;
  }
  a.cert_stats = h->cert_stats;
  return a;
}

int candidate_scratch(flacenc_hip_handle* h, size_t n_rows, uint32_t block_size, bool lpc, bool fixed, bool with_minmax,
                      Candidates* out) {
  const size_t records = n_rows * sizeof(flacenc_hip_subframe_params), rows = n_rows * padded_stride(block_size) * 4;
  int rc;
  if (lpc) {
    if ((rc = ensure(h, h->d_cparams, records)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_cresid, rows)) != FLACENC_HIP_OK) return rc;
    if (with_minmax && (rc = ensure(h, h->d_minmax, n_rows * 2 * sizeof(int32_t))) != FLACENC_HIP_OK) return rc;
    out->lpc_params = static_cast<flacenc_hip_subframe_params*>(h->d_cparams.ptr);
    out->lpc_residual = static_cast<int32_t*>(h->d_cresid.ptr);
    out->minmax = with_minmax ? static_cast<int32_t*>(h->d_minmax.ptr) : nullptr;
  }
  if (fixed) {
    if ((rc = ensure(h, h->d_fparams, records)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_fresid, rows)) != FLACENC_HIP_OK) return rc;
    if ((rc = ensure(h, h->d_fkeys, n_rows * 8)) != FLACENC_HIP_OK) return rc;
    out->fixed_params = static_cast<flacenc_hip_subframe_params*>(h->d_fparams.ptr);
    out->fixed_residual = static_cast<int32_t*>(h->d_fresid.ptr);
    out->fixed_keys = static_cast<unsigned long long*>(h->d_fkeys.ptr);
  }
  return FLACENC_HIP_OK;
}

// What scratch_grant gives a record.  The split scratch: R[] and the predictor records between the launches of the split
// pipelines, and the counter through which bigblock_residual_kernel tells the clean-up launch whether it marked anything
// (QlpcKernelArgs::marked_count).  The pipeline's own counter is cleared on its stream here: a pipeline that attached this
// scratch but had no clean-up launch behind it (the fused 4096 / 4608 kernels, for one) leaves its count and list entries
// in the other slot, and the pipeline after the next one would otherwise start from them and visit records twice.
int attach_scratch(flacenc_hip_handle* h, QlpcKernelArgs& a, ScratchGrant grant, hipStream_t stream) {
  int rc;
  if (grant.sumabs) {  // (launch_qlpc runs sumabs_reference_kernel when `sumabs_scratch` is set)
    if ((rc = ensure(h, h->d_sumabs, static_cast<size_t>(a.n_subframes) * 5 * 64 * sizeof(float))) != FLACENC_HIP_OK) return rc;
    a.sumabs_scratch = static_cast<float*>(h->d_sumabs.ptr);
  }
  if (!grant.split) return FLACENC_HIP_OK;
  if ((rc = ensure(h, h->d_split, static_cast<size_t>(a.n_subframes) * (33 * 8 + 36 * 4))) != FLACENC_HIP_OK) return rc;
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
  HIP_TRY(h, hipMemsetAsync(a.marked_count, 0, 4, stream));
  return FLACENC_HIP_OK;
}

// The order mode of the certified shapes (order_mode_core.h has the rule and its reasons): the HIP calls around its step
int launch_adaptive(flacenc_hip_handle* h, const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, hipStream_t stream) {
  flacenc_hip_handle::OrderMode& om = h->adaptive;
  order_mode::Step st{false, false, 0u};
  if (plan_qlpc_route(a).order == QlpcRoute::kCertifiedFused && om.enabled != 0 && h->cert_stats == nullptr &&
      a.autocorr == nullptr && a.lpc_coefs == nullptr && a.n_subframes < order_mode::kFeedbackMaxSubframes) {
    if (om.d_counters == nullptr) {
      HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&om.d_counters), 16));
      HIP_TRY(h, hipMemset(om.d_counters, 0, 16));
      HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&om.verdict), 8, hipHostMallocMapped));
      *om.verdict = 0ull;
    }
    // (the latest verdict that has landed, a plain read of the pinned word: late is fine, torn it cannot be)
    st = order_mode::step(om.state, *reinterpret_cast<volatile unsigned long long*>(om.verdict), a.n_subframes);
  }
  QlpcKernelArgs b = a;
  if (st.two_pass) {
    b.certify = 0;
    b.reference_order = 1u;  // (the autocorrelation alone: the selector's sums follow sumabs_scratch, which the flags decide)
    int rc;  // (lazily: certified launches, the rule, never pay for the split scratch)
    if (b.split_scratch == nullptr && (rc = attach_scratch(h, b, {true, false}, stream)) != FLACENC_HIP_OK) return rc;
  } else if (st.carry) {
    b.cert_stats = om.d_counters;
  }
  HIP_TRY(h, launch_qlpc(b, plan, stream));
  if (st.feedback != 0u) {
    unsigned long long* out = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&out), om.verdict, 0));
    hipLaunchKernelGGL(cert_feedback_kernel, dim3(1), dim3(1), 0, stream, om.d_counters, out, st.feedback);
    HIP_TRY(h, hipGetLastError());
  }
  return FLACENC_HIP_OK;
}

// FLACENC_HIP_FLAG_RICE_ESCAPE: the post-pass over the records and rows a candidate batch has just enqueued
// (rice_escape.cpp)
int enqueue_rice_escape(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, const CandidateBatch& b, hipStream_t stream) {
  flacenc_hip::RiceEscapeArgs e{};
  e.params = b.params;
  e.residual = b.residual;
  e.residual_stride = b.residual_stride;
  e.block_size = b.block_size;
  e.n_rows = static_cast<uint32_t>(b.n_subframes);
  e.max_rice_parameter = q.max_rice_parameter;
  e.finest_only = (q.flags & FLACENC_HIP_FLAG_FINEST_RICE_ORDER) ? 1u : 0u;
  HIP_TRY(h, flacenc_hip::launch_rice_escape(e, stream));
  return FLACENC_HIP_OK;
}

namespace {
// What both batches start from: the launch plan at `order`, checked against the LDS; base_args with the batch's rows and
// outputs; the bit tables' scratch of blocks above 16384 samples
int batch_record(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, const WindowEntry* win, uint32_t order,
                 const CandidateBatch& b, QlpcLaunchPlan* plan, QlpcKernelArgs* out) {
  *plan = plan_qlpc_launch(b.block_size, order);
  if (plan->smem_bytes > 160 * 1024) {
    h->last_error = "internal: LDS plan exceeds 160 KiB";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  QlpcKernelArgs a = base_args(h, q, win, b.samples, b.stride, b.block_size, b.n_subframes, b.bps, b.bps_uniform, b.stereo);
  a.params = b.params;
  a.residual = b.residual;
  a.residual_stride = b.residual_stride;
  if (plan->table_scratch_bytes_per_subframe) {
    int rc = ensure(h, h->d_tables, plan->table_scratch_bytes_per_subframe * b.n_subframes);
    if (rc != FLACENC_HIP_OK) return rc;
    a.table_scratch = static_cast<uint32_t*>(h->d_tables.ptr);
  }
  *out = a;
  return FLACENC_HIP_OK;
}

int enqueue_lpc(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, CandidateBatch& b, hipStream_t stream) {
  b.placed = false;
  const uint32_t block_size = b.block_size;
  const size_t n_subframes = b.n_subframes;
  flacenc_hip_qlpc_config qcfg = *cfg;
  qcfg.flags = search_flags(!h->lpc_windows.empty(), h->precision_floor, cfg->flags, cfg->quant_precision);
  cfg = &qcfg;
  const WindowEntry* win = nullptr;
  int rc = get_window(h, cfg, block_size, &win);
  if (rc != FLACENC_HIP_OK) return rc;
  const float* const win_dev = win->dev;  // (get_window_entry may grow h->windows below)
  QlpcLaunchPlan plan;
  QlpcKernelArgs a;
  if ((rc = batch_record(h, *cfg, win, cfg->lpc_order, b, &plan, &a)) != FLACENC_HIP_OK) return rc;
  a.autocorr = b.autocorr;
  a.lpc_coefs = b.lpc_coefs;
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
  const bool order_search = lpc_search(cfg->flags);
  if ((rc = attach_scratch(h, a, scratch_grant(a, LaunchKind::kLpcBatch, order_search), stream)) != FLACENC_HIP_OK) return rc;
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
  // frame-level callers on the big-block shapes (only bigblock_residual_kernel knows how) ...
  if (b.stereo && b.minmax_out != nullptr && (bigblock_eligible(a) || (a.direct_mse && bigblock_shape_eligible(a)))) {
    if (b.analyse_only) {
      // ... no rows at all: records and the roles' min / max only (the deciding store pass, bigblock_residual_kernel's
      // mode 2, produces the two rows the frame keeps)
      a.residual_mode = 1u;
      b.placed = true;
    } else if (b.residual_lr != nullptr && (reinterpret_cast<uintptr_t>(b.residual_lr) & 15) == 0 && (b.residual_lr_stride & 3) == 0) {
      // ... L / R candidates straight into the output rows, role min / max from the residual kernel
      a.residual_lr = b.residual_lr;
      a.residual_lr_stride = b.residual_lr_stride;
      b.placed = true;
    }
    if (b.placed) a.minmax_out = b.minmax_out;
  }
  return launch_adaptive(h, a, plan, stream);
}
}  // namespace

// The one exit of the LPC candidates.  Under FLACENC_HIP_FLAG_RICE_ESCAPE every record and row goes to `params` /
// `residual` (no rows placed in the caller's frame; plan_frame_call asks for no analyse-only launch) and the escape pass
// runs behind them -- on the winner's record where a search flag chose one.
int enqueue(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, CandidateBatch& b, hipStream_t stream) {
  if (!(cfg->flags & FLACENC_HIP_FLAG_RICE_ESCAPE)) return enqueue_lpc(h, cfg, b, stream);
  b.placed = false;
  CandidateBatch plain = b;
  plain.residual_lr = plain.minmax_out = nullptr;
  int rc = enqueue_lpc(h, cfg, plain, stream);
  if (rc != FLACENC_HIP_OK) return rc;
  return enqueue_rice_escape(h, *cfg, b, stream);
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
int enqueue_fixed(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, CandidateBatch& b, hipStream_t stream) {
  int rc = verify_fixed(h, cfg);
  if (rc != FLACENC_HIP_OK) return rc;
  const size_t n_subframes = b.n_subframes;
  // FLACENC_HIP_FLAG_RICE_ESCAPE: the pass runs on the selected order's record; the selector's keys (and BitCount's
  // comparison of unescaped code_bits) are what they are without the flag.  (plan_frame_call: never analyse-only.)
  auto escape = [&]() -> int {
    return (cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE) ? enqueue_rice_escape(h, cfg->qlpc, b, stream) : FLACENC_HIP_OK;
  };
  QlpcLaunchPlan plan;
  QlpcKernelArgs a;
  if ((rc = batch_record(h, cfg->qlpc, nullptr, 4, b, &plan, &a)) != FLACENC_HIP_OK) return rc;
  fixed_batch_fields(a, *cfg);
  a.fixed_keys = h->fixed_keys;
  a.selector_keys = b.selector_keys;
  if ((rc = attach_scratch(h, a, scratch_grant(a, LaunchKind::kFixedBatch), stream)) != FLACENC_HIP_OK) return rc;
  if (a.fixed_mode == 1) {  // ApproxEnt
    if (b.analyse_only) a.residual_mode = 1u;  // (plan_frame_call asked bigblock_fixed_eligible of this record)
    HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
    return escape();
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
                     static_cast<uint8_t*>(h->d_sel.ptr), b.selector_keys);
  HIP_TRY(h, hipGetLastError());
  a.fixed_mode = 3;
  a.forced_orders = static_cast<const uint8_t*>(h->d_sel.ptr);
  a.selector_keys = nullptr;
  HIP_TRY(h, flacenc_hip::launch_qlpc(a, plan, stream));
  return escape();
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
  CandidateBatch b(samples, n_subframes, block_size, stride, bps);
  b.write_to(params, residual, residual_stride);
  b.autocorr = autocorr;
  b.lpc_coefs = lpc_coefs;
  return enqueue(h, cfg, b, static_cast<hipStream_t>(stream));  // NULL = HIP's default (null) stream
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
    return drained(h, flacenc_hip_qlpc_batch_async(h, cfg, samples, n_subframes, block_size, stride, bps, params, residual,
                                                   residual_stride, autocorr, lpc_coefs, h->stream), false);
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
  rc = flacenc_hip_qlpc_batch_async(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), n_subframes, block_size, dstride,
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
  if ((rc = check_bits_per_sample(h, bits_per_sample)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  CandidateBatch b(frames, n_frames * 4, block_size, stride);
  b.write_to(params, residual, residual_stride);
  b.stereo = true;
  b.bps_uniform = bits_per_sample;
  return enqueue(h, cfg, b, static_cast<hipStream_t>(stream));  // NULL = HIP's default (null) stream
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
  CandidateBatch b(samples, n_sub, block_size, stride, stereo ? nullptr : bps);
  b.write_to(params, residual, residual_stride);
  b.stereo = stereo;
  b.bps_uniform = bits_per_sample;
  b.selector_keys = reinterpret_cast<unsigned long long*>(selector_keys);
  return enqueue_fixed(h, cfg, b, static_cast<hipStream_t>(stream));
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
