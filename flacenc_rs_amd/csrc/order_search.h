// order_search.h -- FLACENC_HIP_FLAG_ORDER_SEARCH, FLACENC_HIP_FLAG_WINDOW_SEARCH and FLACENC_HIP_FLAG_PRECISION_SEARCH:
// the LPC predictor of every QLPC candidate subframe chosen by an exhaustive search over candidates (window j, order o,
// precision q0 - i) -- the analysis windows 0..W-1, with the order search every order 1..P, with the precision search
// every precision from quant_precision down to the handle's floor (DESIGN.md sections 4.10, 4.11, 4.16) -- in front of
// the stage-3 residual kernels.
#ifndef FLACENC_HIP_ORDER_SEARCH_H_
#define FLACENC_HIP_ORDER_SEARCH_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "qlpc_kernel.h"

namespace flacenc_hip {

constexpr uint32_t kMaxSearchWindows = 8;  // FLACENC_HIP_MAX_LPC_WINDOWS
// Bound of the search scratch of one call: steps 1..4 below run over slices of at most this many bytes' worth of
// subframes (the handle's growth slack on top keeps the allocation below 1 GiB).
constexpr size_t kSearchScratchCap = static_cast<size_t>(768) << 20;

// The candidates of one flagged candidate batch: W analysis windows (window 0 the config's), and the orders searched
// per window (P with FLACENC_HIP_FLAG_ORDER_SEARCH, else 1: lpc_order only).
struct SearchShape {
  const float* windows[kMaxSearchWindows];  // device weight tables (32 leading pad floats), nullptr = all ones
  uint32_t n_windows;                       // W, 1..8
  uint32_t search_orders;                   // 1: orders 1..P per window; 0: order P only
  // FLACENC_HIP_FLAG_ORDER_GUESS: K in 1..32 -- of the orders 1..P (search_orders = 1) the search codes only (0, P) and
  // every window's K guesses (order_guess_core.h); 0: every candidate
  uint32_t guess_orders;
  // FLACENC_HIP_FLAG_PRECISION_SEARCH: Q in 1..quant_precision -- every (window, order) is coded at the precisions
  // quant_precision - i, i = 0..Q-1; 1: at quant_precision only.  Candidate (j, o, i) has the index
  // (j * Pc + oi) * Q + i, so the lower index is the lower window, then the lower order, then the higher precision.
  uint32_t n_precisions;
  // flacenc_hip_debug_set_order_guess_trace (tests): device, nullable -- every order_guess_kernel lane's record, 264
  // bytes each, at [(subframe of the call) * W + window]
  void* guess_trace;
};

// Handle scratch of a flagged candidate batch of n subframes at lpc_order P: per subframe R[0..32] of every window
// ([W][33] f64, 264 B each), the C = W x (P or 1) x Q candidate predictor records ([C][36] int32: qc[32], order, shift,
// status, precision; 144 B each) and the chosen candidate (uint32), with the order guess also k_o of every (window,
// order) ([W x P] f64) -- for the largest slice the call runs, so never above kSearchScratchCap.
size_t order_search_scratch_bytes(uint32_t n_subframes, uint32_t lpc_order, const SearchShape& shape);

// The whole flagged pipeline of a candidate batch `a` (split scratch attached; autocorr / lpc_coefs as the caller asked),
// steps 1..4 per slice of subframes:
//   1. R[0..P] of every window in the stable build's order (nightly's with `nightly`);
//   2. order_levinson_kernel: levinson_quantize at every (j, o), one lane per (subframe, window, order), which writes
//      the Q records of its precisions from the one recursion;
//      with the order guess then order_guess_kernel, one lane per (subframe, window): every candidate but (0, P) and the
//      window's K guesses gets a status the search skips, at every precision;
//   3. order_search_kernel: one workgroup per subframe, every candidate's residual and exact Rice search -> the
//      candidate whose Lpc::count_bits -- with the candidate's own precision -- is smallest (ties: the lower window,
//      then the lower order, then the higher precision; no candidate with status 0: (0, P, quant_precision));
//   4. order_pick_kernel: the chosen candidate's predictor record (and unquantised coefficients into a.lpc_coefs, its
//      window's R[] into a.autocorr);
// then over the whole batch
//   5. the stage-3 kernels write the records and residual rows from those predictors (a predictor record's word 35,
//      when not 0, is the subframe's precision in place of the launch's: Q > 1 only).
hipError_t launch_order_search(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, uint32_t nightly,
                               const SearchShape& shape, void* scratch, hipStream_t stream, uint32_t* n_slices = nullptr);
// (n_slices, when given: how many slices of at most kSearchScratchCap the call cut its subframes into)

}  // namespace flacenc_hip
#endif
