// order_search.h -- FLACENC_HIP_FLAG_ORDER_SEARCH: the LPC order of every QLPC candidate subframe chosen by an exhaustive
// search over orders 1..P, in front of the unflagged stage-3 residual kernels.
#ifndef FLACENC_HIP_ORDER_SEARCH_H_
#define FLACENC_HIP_ORDER_SEARCH_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "qlpc_kernel.h"

namespace flacenc_hip {

// Handle scratch of one flagged candidate batch of n subframes at lpc_order P: the P candidate predictor records
// ([n][P][36] int32: qc[32], order, shift, status, 0) and the chosen order per subframe ([n] uint32).
size_t order_search_scratch_bytes(uint32_t n_subframes, uint32_t lpc_order);

// The whole flagged pipeline of a candidate batch `a` (split scratch attached; autocorr / lpc_coefs as the caller asked):
//   1. R[0..P] in the stable build's order (nightly's with `nightly`) into a.autocorr or the split scratch;
//   2. order_levinson_kernel: levinson_quantize at every order o = 1..P, one lane per (subframe, o);
//   3. order_search_kernel: one workgroup per subframe, every candidate's residual and exact Rice search -> the order whose
//      Lpc::count_bits is smallest (ties: the lower order; no candidate with status 0: order P);
//   4. order_pick_kernel: the chosen order's predictor record (and unquantised coefficients into a.lpc_coefs);
//   5. the unflagged stage-3 kernels write the records and residual rows from that predictor.
hipError_t launch_order_search(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, uint32_t nightly, void* scratch,
                               hipStream_t stream);

}  // namespace flacenc_hip
#endif
