// qlpc_dispatch.cpp -- launch planning (workgroup size, LDS budget, order bucket), the route of a launch
// (plan_qlpc_route: which kernels run, in one pure step) and its run over the kernel instantiations (launch_qlpc).
#include "qlpc_kernel.h"

#include "acorr_reference.h"
#include "direct_mse.h"
#include "sumabs_reference.h"

namespace flacenc_hip {
namespace {

constexpr int kLeadRows = 2;
constexpr int kMiscCount = 16;

int bucket_order(int P) {
  if (P <= 8) return 8;
  if (P <= 10) return 10;
  if (P <= 12) return 12;
  if (P <= 16) return 16;
  if (P <= 24) return 24;
  return 32;
}

}  // namespace

// rows the vector loads and stores of every kernel but the generic one need: 16-byte aligned, whole dwordx4 strides, and
// the four roles of every stereo frame present
bool rows_aligned(const QlpcKernelArgs& a) {
  if ((reinterpret_cast<uintptr_t>(a.samples) & 15) || (a.stride & 3)) return false;
  if ((reinterpret_cast<uintptr_t>(a.residual) & 15) || (a.residual_stride & 3)) return false;
  return !(a.stereo && (a.n_subframes & 3));
}

bool wave_kernel_eligible(const QlpcKernelArgs& a) {
  if ((a.block_size != 4096 && a.block_size != 4608) || a.lpc_order > 12) return false;
  if (a.block_size == 4608 && a.pack_out != nullptr) return false;  // (the fused bit writer exists for 4096 only)
  if (a.fixed_mode != 0) return false;  // fixed_lpc as a stand-alone batch: generic kernel
  if (a.direct_mse) return false;       // experimental estimators: direct_mse_kernel + the split pipeline
  return !a.force_generic && rows_aligned(a);
}

bool cert_shape(const QlpcKernelArgs& a) {
  return (a.block_size == 4096 || a.block_size == 4608) && a.lpc_order >= 1 && a.lpc_order <= 12;
}

bool subwave_shape(uint32_t n) {
  return n == 256 || n == 512 || n == 1024 || n == 2048 || n == 288 || n == 576 || n == 1152 || n == 2304;
}

static bool subwave_buffers_ok(const QlpcKernelArgs& a) {
  if (!subwave_shape(a.block_size) || a.n_subframes == 0 || a.force_generic || a.only_marked || a.direct_mse) return false;
  if (a.sumabs_in != nullptr || a.lpc_stage != 0) return false;
  if (!rows_aligned(a)) return false;
  return a.marked_count != nullptr && a.pack_out == nullptr;
}

// the estimator's partitions: a whole number of the selector's sub-sums (an eighth of a lane's samples), and either
// 1 / 2 / 4 per lane or a power-of-two group of lanes inside the segment
static bool subwave_fixed_ok(const QlpcKernelArgs& a) {
  if (a.fixed_order_sel != 1u || a.fixed_max_order > 4u || a.fixed_partitions == 0u) return false;
  const uint32_t n = a.block_size, spl = (n % 72u) == 0 ? 72u : 64u, parts = a.fixed_partitions;
  if (n % parts) return false;
  const uint32_t psz = n / parts;
  if (psz < spl) return psz * 2 == spl || psz * 4 == spl;
  const uint32_t lanes = psz / spl;
  return psz % spl == 0 && (lanes & (lanes - 1)) == 0;
}

// the plain analysis (records + residual rows, no on-device decision) in the build's canonical summation order
// (`reference_order`, `have_r`: the record's, or what the pre-passes of its route will have made of them)
static bool subwave_candidates_ok(const QlpcKernelArgs& a, uint32_t reference_order, bool have_r) {
  if (!subwave_buffers_ok(a) || a.lpc_order > 12 || a.lpc_order == 0 || a.fixed_mode != 0) return false;
  // (a flagged summation order reaches the kernel as R[] of the launch in front: acorr_in)
  if (reference_order != 0 && !have_r) return false;
  return a.frame_results == nullptr && a.chan_results == nullptr && a.params != nullptr;
}

bool subwave_fixed_eligible(const QlpcKernelArgs& a) {
  if (!subwave_buffers_ok(a) || a.fixed_mode != 1u || !subwave_fixed_ok(a)) return false;
  if (a.reference_order != 0 || a.acorr_in != nullptr) return false;
  return a.frame_results == nullptr && a.chan_results == nullptr && a.params != nullptr;
}

bool subwave_frame_eligible(const QlpcKernelArgs& a) {
  if (!subwave_buffers_ok(a) || !a.stereo || a.fixed_mode != 0 || a.frame_results == nullptr) return false;
  if (a.reference_order != 0 || a.acorr_in != nullptr) return false;  // (flagged orders: the selector's sums are the reference's too)
  if (!a.use_lpc || a.lpc_order > 12 || a.lpc_order == 0) return false;
  return !a.use_fixed || subwave_fixed_ok(a);
}

bool subwave_channels_eligible(const QlpcKernelArgs& a) {
  if (!subwave_buffers_ok(a) || a.stereo || a.fixed_mode != 0 || a.chan_results == nullptr) return false;
  if (a.reference_order != 0 || a.acorr_in != nullptr) return false;
  if (!a.use_lpc || a.lpc_order > 12 || a.lpc_order == 0) return false;
  return !a.use_fixed || subwave_fixed_ok(a);
}

// fixed_lpc with OrderSel::ApproxEnt on the same shapes: estimator partitions that are whole groups of lanes
bool bigblock_fixed_eligible(const QlpcKernelArgs& a) {
  if (a.fixed_mode != 1u || a.lpc_stage != 0 || a.force_generic) return false;
  if (a.block_size != 4096 && a.block_size != 8192 && a.block_size != 16384) return false;
  const uint32_t parts = a.fixed_partitions;
  if (parts == 0 || (parts & (parts - 1)) != 0) return false;
  const uint32_t psize = a.block_size / parts;
  if (psize < 64 || psize > 4096) return false;
  if (a.fixed_max_order > 4) return false;
  if (a.frame_results || a.chan_results || a.pack_out) return false;
  return rows_aligned(a) && a.split_scratch != nullptr;
}

bool bigblock_eligible(const QlpcKernelArgs& a) {
  // (4096 at orders 13..32 too: below 13 the fused 4096 kernel has it, above it would fall to the generic one;
  // 8192 / 16384 at every order -- round 2 left orders up to 12 on those blocks to the generic kernel, 88 G
  // samples/s where order 24 ran at 146)
  if (a.lpc_order < 1 || a.lpc_order > 32) return false;
  if (a.lpc_order < 13 && a.block_size == 4096) return false;
  return bigblock_shape_eligible(a);
}

bool bigblock_shape_eligible(const QlpcKernelArgs& a) {
  if (a.block_size != 4096 && a.block_size != 8192 && a.block_size != 16384) return false;
  if (a.lpc_order < 1 || a.lpc_order > 32) return false;
  if (a.fixed_mode != 0 || a.lpc_stage != 0 || a.force_generic) return false;
  if (a.frame_results || a.chan_results || a.pack_out) return false;
  return rows_aligned(a) && a.split_scratch != nullptr;
}

// ---- the launchers, each per-instance list expanded once ----

namespace {

int bucket12(uint32_t order) { return order <= 8 ? 8 : (order <= 10 ? 10 : 12); }

// the predictor records of the split pipelines: behind the [n][33] doubles of R[] in the split scratch
int32_t* pred_records(const QlpcKernelArgs& a) {
  return reinterpret_cast<int32_t*>(reinterpret_cast<double*>(a.split_scratch) + static_cast<size_t>(a.n_subframes) * 33);
}

// the generic kernel's instance for `plan`
hipError_t launch_generic(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, hipStream_t stream) {
#define FLACENC_HIP_CASE(MP, BG) \
  if (plan.maxp == MP && plan.big == (BG != 0)) return launch_qlpc_##MP##_##BG(a, plan.threads, plan.smem_bytes, stream);
  FLACENC_HIP_FOR_EACH_INSTANCE(FLACENC_HIP_CASE)
#undef FLACENC_HIP_CASE
  return hipErrorInvalidValue;
}

// levinson_batch_kernel (one subframe per lane): a.autocorr -> a.pred_out
hipError_t launch_levinson(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, hipStream_t stream) {
#define FLACENC_HIP_LEV(MP, BG) \
  if (plan.maxp == MP && plan.big == (BG != 0)) return launch_levinson_##MP##_##BG(a, stream);
  FLACENC_HIP_FOR_EACH_INSTANCE(FLACENC_HIP_LEV)
#undef FLACENC_HIP_LEV
  return hipErrorInvalidValue;
}

// qlpc_subwave_kernel's instance for the record's shape, order bucket `mp` and variant
hipError_t launch_subwave(const QlpcKernelArgs& a, int mp, int var, hipStream_t stream) {
  const int st = a.stereo ? 1 : 0;
  const int spl = (a.block_size % 72u) == 0 ? 72 : 64;
#define FLACENC_HIP_SUBCASE(MP, ST, SP, V) \
  if (mp == MP && st == ST && spl == SP && var == V) return launch_qlpc_subwave_##MP##_##ST##_##SP##_##V(a, stream);
  FLACENC_HIP_FOR_EACH_SUBWAVE_INSTANCE(FLACENC_HIP_SUBCASE)
#undef FLACENC_HIP_SUBCASE
  return hipErrorInvalidValue;
}

// the fused kernel for blocks of 4096 / 4608 samples
hipError_t launch_fused(const QlpcKernelArgs& a, int mp, int variant, hipStream_t stream) {
  if (a.block_size == 4608) {
#define FLACENC_HIP_W72CASE(MP, ST) \
  if (mp == MP && variant == ST) return launch_qlpc_wave72_##MP##_##ST(a, stream);
    FLACENC_HIP_FOR_EACH_WAVE72_INSTANCE(FLACENC_HIP_W72CASE)
#undef FLACENC_HIP_W72CASE
    return hipErrorInvalidValue;
  }
#define FLACENC_HIP_WCASE(MP, ST) \
  if (mp == MP && variant == ST) return launch_qlpc_wave_##MP##_##ST(a, stream);
  FLACENC_HIP_FOR_EACH_WAVE_INSTANCE(FLACENC_HIP_WCASE)
#undef FLACENC_HIP_WCASE
  return hipErrorInvalidValue;
}

// R[] of the subframes of `a` in the reference's order (acorr_reference_mfma_kernel; `nightly`: simd-nightly's) into
// `out` -- of every subframe, or (`marked`) of the records the sub-wave kernel's order certificate marked with status -2
hipError_t reference_chains(const QlpcKernelArgs& a, double* out, bool nightly, bool marked, hipStream_t stream) {
  AcorrRefArgs r{};
  r.samples = a.samples;
  r.stride = a.stride;
  r.block_size = a.block_size;
  r.n_subframes = a.n_subframes;
  r.stereo = a.stereo;
  r.window = a.window;
  r.lpc_order = a.lpc_order;
  r.nightly = nightly ? 1u : 0u;
  r.out = out;
  if (marked) {
    r.marked_params = a.params;
    r.marked_count = a.marked_count;
    r.marked_list = a.marked_list;
    r.marked_cap = a.marked_cap;
    r.marked_unit = a.marked_unit;
  }
  return launch_acorr_reference(r, stream);
}

}  // namespace

hipError_t launch_stage3(QlpcKernelArgs s3, const int32_t* pred, bool bigblock, const QlpcLaunchPlan& plan,
                         hipStream_t stream) {
  s3.lpc_stage = 3;
  s3.pred = pred;
  s3.autocorr = nullptr;
  s3.lpc_coefs = nullptr;  // written with the predictor record
  s3.acorr_in = nullptr;
  if (bigblock) {
    if (hipError_t err = launch_bigblock_residual(s3, stream); err != hipSuccess) return err;
    // clean-up launch: the generic kernel redoes the subframes the big-block kernel marked (residuals
    // of 2^26 and more need the literal chunk-clamped bit tables); every other workgroup exits at once
    s3.only_marked = 1;
  }
  return launch_generic(s3, plan, stream);
}

hipError_t launch_subwave_frames(const QlpcKernelArgs& a, hipStream_t stream) {
  QlpcKernelArgs r = a;
  if (a.cert_subwave != 0u && a.acorr_in == nullptr) {
    // the two-pass form of the unflagged order on these shapes: the reference's chains for every QLPC candidate in front,
    // the kernel's own autocorrelation skipped (the fixed-LPC candidate keeps the canonical sums of the unflagged mode)
    if (a.split_scratch == nullptr) return hipErrorInvalidValue;
    double* racc = reinterpret_cast<double*>(a.split_scratch);
    if (hipError_t err = reference_chains(a, racc, false, false, stream); err != hipSuccess) return err;
    r.acorr_in = racc;
  }
  return launch_subwave(r, bucket12(a.lpc_order), a.stereo ? 2 : 3, stream);
}

QlpcLaunchPlan plan_qlpc_launch(uint32_t block_size, uint32_t lpc_order) {
  QlpcLaunchPlan plan;
  const int n = static_cast<int>(block_size);
  const int rows = (n + 15) / 16;
  plan.big = n > 16384;
  plan.maxp = bucket_order(static_cast<int>(lpc_order));
  if (plan.big) plan.maxp = plan.maxp <= 12 ? 12 : 32;
  // must match the kernel's __launch_bounds__
  const int max_threads = plan.maxp <= 12 ? 1024 : (plan.maxp <= 16 ? 512 : 256);
  int threads = 64;
  while (threads < rows && threads < max_threads) threads <<= 1;
  // a block a little over half a workgroup's worth of 16-sample rows (1152 = 72 rows, 2304 = 144) takes the smaller
  // workgroup and a second, mostly idle chunk round: the second wave's idle lanes cost issue slots in every phase,
  // the extra round only in two (measured: 2304 at order 8 / 10 78 -> 90 / 59 -> 82 G samples/s, 1152 at order 10 56 -> 65)
  if (n < 4096 && threads > 64 && rows <= threads / 2 + threads / 8) threads >>= 1;
  plan.threads = threads;
  const int J = (rows + threads - 1) / threads;
  int Jp = 1;
  while (Jp < J) Jp <<= 1;
  const int W = threads / 64;
  const int rowstride = plan.big ? 16 : 20;
  size_t bytes = static_cast<size_t>(rows + kLeadRows) * rowstride * 4;
  bytes += static_cast<size_t>(Jp) * W * (plan.maxp + 1) * 8;
  bytes = (bytes + 15) & ~static_cast<size_t>(15);
  bytes += 40 * 8 + 16 * 8 + 32 * 4 + kMiscCount * 4;
  bytes += (5 * 64 + 16) * 8;  // kFixedSumWords (qlpc_kernel_impl.h): fixed-LPC order selection
  if (!plan.big) {
    // finest_partition_order, rice.rs:157-165 (warm-up <= 32 < 64)
    int lg = 31 - __builtin_clz(static_cast<unsigned>(n / 64));
    int tz = __builtin_ctz(static_cast<unsigned>(n));
    int fo = lg < tz ? lg : tz;
    if (fo > 8) fo = 8;
    bytes += static_cast<size_t>(((2 << fo) + 15) & ~15);  // the levels' Rice parameters, 2 bytes per finest partition
    bytes += static_cast<size_t>(1 << fo) * 32 * 4;
  } else {
    bytes += 2 * FLACENC_HIP_MAX_RICE_PARTITIONS;
  }
  plan.smem_bytes = bytes;
  plan.table_scratch_bytes_per_subframe =
      plan.big ? static_cast<size_t>(FLACENC_HIP_MAX_RICE_PARTITIONS) * 32 * 4 : 0;
  return plan;
}

// The launches of one launch_qlpc call, decided in one step from the record as the caller filled it (no HIP call, nothing
// allocated): launch_qlpc below runs exactly this, in this order, and the comments there say why.
QlpcRoute plan_qlpc_route(const QlpcKernelArgs& a) {
  QlpcRoute rt{};
  const bool wave = wave_kernel_eligible(a);
  const bool analysis = a.fixed_mode == 0 && a.lpc_stage == 0;  // QLPC analysis from the samples on
  rt.direct_mse = a.direct_mse && analysis;
  // 1. the summation order of R[]
  rt.certify = a.certify != 0u;
  rt.reference_order = a.reference_order;
  if (a.certify != 0u && !rt.direct_mse) {
    // (FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY: the stable order is asked for, but only for the integers -- the certificate
    // gives those; reference_order stays set for the fixed-LPC selector's sums)
    const bool order_ok = a.reference_order == 0u || (a.reference_order == 1u && a.integer_parity_only != 0u);
    const bool shape = cert_shape(a) && order_ok && !a.direct_mse && analysis && a.acorr_in == nullptr && !a.only_marked;
    const bool two_pass = a.reference_order == 0u && !a.direct_mse && analysis && a.acorr_in == nullptr && !a.only_marked &&
                          a.lpc_order >= 1 && a.split_scratch != nullptr;
    if (shape && wave && a.pack_out == nullptr) {
      rt.order = QlpcRoute::kCertifiedFused;
    } else {
      rt.certify = false;
      if (shape || two_pass) {
        rt.order = QlpcRoute::kReferencePass;
        rt.reference_order = 1u;
      }
    }
  }
  const bool stable_by_default = rt.reference_order == 0u && !a.direct_mse &&
                                 (a.block_size == 4096u || a.block_size == 8192u || a.block_size == 16384u) &&
                                 a.lpc_order >= 16u && a.split_scratch != nullptr;
  // 2. the pre-passes
  if (rt.reference_order && a.sumabs_in == nullptr && a.sumabs_scratch != nullptr && a.lpc_stage == 0 &&
      (a.fixed_mode == 1u || (a.fixed_mode == 0 && a.use_fixed && a.fixed_order_sel == 1u && (a.frame_results || a.chan_results)))) {
    const bool walk = a.fixed_mode == 0 && a.sumabs_mode == 0 && a.bps == nullptr && a.bps_uniform <= 16u && a.pack_out == nullptr;
    rt.sumabs = walk ? QlpcRoute::kFusedWalk : QlpcRoute::kSumAbsChains;
  }
  rt.chains_marked = !rt.direct_mse && a.only_marked && a.cert_subwave != 0u && a.acorr_marked == nullptr &&
                     a.fixed_mode == 0 && a.split_scratch != nullptr && a.params != nullptr;
  rt.chains_all = !rt.direct_mse && (rt.reference_order || stable_by_default) && rt.order != QlpcRoute::kCertifiedFused &&
                  analysis && a.acorr_in == nullptr;
  if (rt.chains_all && rt.reference_order == 0u) rt.order = QlpcRoute::kStableByDefault;
  const bool have_r = a.acorr_in != nullptr || rt.chains_all;
  // 3. the kernel family
  const bool subwave = subwave_candidates_ok(a, rt.reference_order, have_r);
  if (a.n_subframes == 0) {
    rt.family = QlpcRoute::kNothing;
  } else if ((a.frame_results || a.chan_results) && !wave) {
    rt.family = QlpcRoute::kUnsupported;
  } else if (rt.direct_mse) {
    rt.family = QlpcRoute::kStage3;
    rt.bigblock = bigblock_shape_eligible(a);
  } else if (bigblock_fixed_eligible(a)) {
    rt.family = QlpcRoute::kBigBlockFixed;
  } else if (bigblock_eligible(a) || (have_r && !wave && !subwave && a.lpc_stage == 0)) {
    rt.family = QlpcRoute::kBigBlock;
    rt.bigblock = bigblock_eligible(a);
    rt.bigblock_acorr = !have_r;
  } else if (subwave || subwave_fixed_eligible(a)) {
    rt.family = QlpcRoute::kSubwave;
    rt.variant = a.fixed_mode == 1u ? 1 : 0;
    rt.bucket = rt.variant == 1 ? 8 : bucket12(a.lpc_order);
  } else if (wave) {
    rt.family = QlpcRoute::kFused;
    rt.bucket = bucket12(a.lpc_order);
    rt.variant = a.stereo ? (a.frame_results ? (a.pack_out ? 5 : (a.use_fixed ? 3 : 2)) : 1) : (a.chan_results ? 4 : 0);
    // the instances with the chain walk
    if ((a.sumabs_mode != 0u || rt.sumabs == QlpcRoute::kFusedWalk) && (rt.variant == 3 || rt.variant == 4)) rt.variant += 3;
  } else if (analysis && a.lpc_order >= 16 && a.split_scratch != nullptr) {
    rt.family = QlpcRoute::kSplit;
  } else {
    rt.family = QlpcRoute::kGeneric;
  }
  rt.cleanup = rt.family == QlpcRoute::kBigBlockFixed || rt.family == QlpcRoute::kSubwave ||
               ((rt.family == QlpcRoute::kBigBlock || rt.family == QlpcRoute::kStage3) && rt.bigblock);
  return rt;
}

hipError_t launch_qlpc(const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, hipStream_t stream) {
  const QlpcRoute route = plan_qlpc_route(a);
  if (route.family == QlpcRoute::kNothing) return hipSuccess;
  if (route.family == QlpcRoute::kUnsupported) return hipErrorNotSupported;
  hipError_t err;
  int32_t* pred = nullptr;
  QlpcKernelArgs r = a;  // the record as the launches see it: each rewrite stands with the step that makes it
  // Blocks of 4096 / 8192 / 16384 samples at orders from 16: the unflagged order IS the reference's stable one -- its
  // chains on the f64 matrix cores cost no more than the chunk tree's fma there (BASELINE configs[2] / [4]; 4096-sample
  // blocks: 344 against 404 us per 50 M samples at order 24), so those shapes emit
  // the stable build's bytes by default (the oracle's orc_default_order_is_stable states the same rule)
  // (a function of the shape alone: unaligned rows or FLACENC_HIP_FLAG_GENERIC_KERNEL change the kernels, not the sums)
  // The unflagged order on blocks of 4096 / 4608 samples at orders up to 12 (the oracle's orc_default_order_is_certified):
  // the fused kernel keeps its own sums where they certify the quantised parameters against the reference's chains and
  // runs those chains itself where not (QlpcKernelArgs::certify).  Launches of these shapes that the fused kernel cannot
  // take (unaligned rows, FLACENC_HIP_FLAG_GENERIC_KERNEL) or that cannot certify inside it (the fused bit writer, which
  // returns bytes alone) are simply given the reference's R[] from acorr_reference_kernel: the same integers -- the
  // reference's -- with R[] and the unquantised coefficients in the reference's own order.
  // Every other shape (round 6): the reference's chains for every subframe in a pass of their own in front of the kernel
  // that takes the shape -- the sub-wave kernel (its autocorrelation skipped: acorr_in; an order certificate inside it was
  // 6-13 % faster on noise-like material and 20 to 140 x slower on music, profiles/r06_subwave_two_pass.txt), the
  // big-block kernels, the generic kernel -- so that the unflagged integers are the stable build's on ANY shape
  // (the oracle's orc_default_order_is_two_pass); FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER keeps the one-pass orders.
  r.certify = route.certify ? a.certify : 0u;
  r.reference_order = route.reference_order;  // (kReferencePass: the stable build's order, by the chains in front below)
  if (route.sumabs == QlpcRoute::kFusedWalk) {
    // the fused kernel on material of at most 16 bits (side channel: 17): its exact sums are the reference's
    // f32 chains unless a partition reaches 2^24, and it walks those itself (QlpcKernelArgs::sumabs_mode)
    r.sumabs_mode = r.reference_order;
    r.sumabs_scratch = nullptr;
  } else if (route.sumabs == QlpcRoute::kSumAbsChains) {
    // Reference summation order for fixed_lpc's ApproxEnt selector: every estimator partition's sum of |e|
    // as find_sum_abs_f32's own f32 chain, one (subframe, partition) per lane; the selecting kernels then
    // read the sums instead of adding them up themselves.
    SumAbsRefArgs s{};
    s.samples = r.samples;
    s.stride = r.stride;
    s.block_size = r.block_size;
    s.n_subframes = r.n_subframes;
    s.stereo = r.stereo;
    s.partitions = r.fixed_mode == 1u ? r.fixed_partitions : (64u >> r.fixed_group_log2);
    s.nightly = r.reference_order == 2u ? 1u : 0u;
    s.out = r.sumabs_scratch;
    if ((err = launch_sumabs_reference(s, stream)) != hipSuccess) return err;
    r.sumabs_in = r.sumabs_scratch;
  }
  if (route.direct_mse) {
    // perform_qlpc's experimental branches (src/coding.rs:337-347): the predictor record comes from
    // direct_mse_kernel, then the residual + Rice kernels of the split pipeline take over
    if (r.split_scratch == nullptr) return hipErrorInvalidValue;
    pred = pred_records(r);
    DirectMseArgs d{};
    d.samples = r.samples;
    d.stride = r.stride;
    d.block_size = r.block_size;
    d.n_subframes = r.n_subframes;
    d.stereo = r.stereo;
    d.window = r.window;
    d.lpc_order = r.lpc_order;
    d.precision = r.precision;
    d.mae_steps = r.mae_steps;
    d.pred_out = pred;
    d.autocorr = r.autocorr;
    d.lpc_coefs = r.lpc_coefs;
    d.weight_scratch = r.irls_weight_scratch;
    d.gram_scratch = r.direct_mse_scratch;
    d.irls_state = (r.mae_steps != 0 && r.direct_mse_scratch != nullptr)
                       ? r.direct_mse_scratch + static_cast<size_t>(r.n_subframes) * direct_mse_gram_stride(r.lpc_order)
                       : nullptr;
    if ((err = launch_direct_mse(d, stream)) != hipSuccess) return err;
    r.direct_mse = 0;
    r.reference_order = 0;  // (the estimator has one summation order; nothing left for the order flags here)
  }
  if (route.chains_marked) {
    // The clean-up launch behind the sub-wave kernel's order certificate (round 6): the records it marked with status -2 take
    // the reference's chains -- acorr_reference_mfma_kernel restricted to them (a wave without such a record returns at once,
    // the launch when nothing was marked) -- and the generic kernel redoes them from that R[] (`acorr_marked`).
    double* racc = reinterpret_cast<double*>(r.split_scratch);
    if ((err = reference_chains(r, racc, false, true, stream)) != hipSuccess) return err;
    r.acorr_marked = racc;
  }
  if (route.chains_all) {
    // Reference summation order: R[] by the lane-per-subframe kernel, then the usual pipeline from
    // Levinson on (below: the fused wave kernel with its phase 1 skipped, the big-block kernels from
    // their second launch, or the generic kernel's three-launch split from its second launch).
    if (r.split_scratch == nullptr) return hipErrorInvalidValue;
    double* racc = r.autocorr ? r.autocorr : reinterpret_cast<double*>(r.split_scratch);
    if ((err = reference_chains(r, racc, r.reference_order == 2u, false, stream)) != hipSuccess) return err;
    r.acorr_in = racc;
    r.autocorr = nullptr;  // already written
  }
  switch (route.family) {
    case QlpcRoute::kStage3:
      return launch_stage3(r, pred, route.bigblock, plan, stream);
    case QlpcRoute::kBigBlockFixed: {
      // fixed_lpc on the big-block shapes: order selection -> predictor record -> the residual + Rice kernel with
      // FixedLpc's bit count; subframes with residuals of 2^26 and more are redone by the generic kernel
      QlpcKernelArgs s1 = r, s3 = r;
      s3.pred = s1.pred_out = pred_records(r);
      if ((err = launch_bigblock_fixed_select(s1, stream)) != hipSuccess) return err;
      s3.selector_keys = nullptr;  // written by the selection
      s3.fixed_keys = nullptr;
      if ((err = launch_bigblock_fixed_residual(s3, stream)) != hipSuccess) return err;
      r.only_marked = 1;
      r.split_scratch = nullptr;
      return launch_generic(r, plan, stream);
    }
    case QlpcRoute::kBigBlock: {
      // R[] -> levinson_batch_kernel (one subframe per lane) -> residual + Rice search
      if (r.split_scratch == nullptr) return hipErrorInvalidValue;
      QlpcKernelArgs s2 = r;
      s2.autocorr = const_cast<double*>(r.acorr_in);
      if (route.bigblock_acorr) {
        s2.autocorr = r.autocorr ? r.autocorr : reinterpret_cast<double*>(r.split_scratch);
        if ((err = launch_bigblock_acorr(s2, stream)) != hipSuccess) return err;
      }
      s2.pred_out = pred_records(r);
      if ((err = launch_levinson(s2, plan, stream)) != hipSuccess) return err;
      return launch_stage3(r, s2.pred_out, route.bigblock, plan, stream);
    }
    case QlpcRoute::kSubwave:
      // several subframes per wave; what it marks (residuals of 2^25 and more, saturated Rice tables) is redone by the
      // generic kernel's clean-up launch, which returns at once when nothing was marked
      if ((err = launch_subwave(r, route.bucket, route.variant, stream)) != hipSuccess) return err;
      r.only_marked = 1;
      r.autocorr = nullptr;  // (written; the clean-up rewrites records and rows only)
      r.lpc_coefs = nullptr;
      if (r.acorr_in != nullptr) {
        // R[] came from the launch in front (the reference's chains of the unflagged order, or a flagged order): what the
        // kernel marked (-2) is redone from that very R[]
        r.acorr_marked = r.acorr_in;
        r.acorr_in = nullptr;
        r.reference_order = 0u;
      }
      return launch_generic(r, plan, stream);
    case QlpcRoute::kFused:
      return launch_fused(r, route.bucket, route.variant, stream);
    case QlpcRoute::kSplit: {
      // Large orders: the recursion is ~5 P^2 / 2 serial instructions, during which a whole workgroup
      // would idle -- run it one subframe per lane between two launches of the generic kernel instead
      // (R[] and the quantised predictor go through `split_scratch`; the samples are read twice).
      QlpcKernelArgs s1 = r, s2 = r, s3 = r;
      s1.lpc_stage = 1;
      s1.autocorr = r.autocorr ? r.autocorr : reinterpret_cast<double*>(r.split_scratch);
      if ((err = launch_generic(s1, plan, stream)) != hipSuccess) return err;
      s2.autocorr = s1.autocorr;
      s2.pred_out = pred_records(r);
      if ((err = launch_levinson(s2, plan, stream)) != hipSuccess) return err;
      s3.lpc_stage = 3;
      s3.pred = s2.pred_out;
      s3.autocorr = nullptr;   // already written by the first launch
      s3.lpc_coefs = nullptr;  // written by the batch kernel
      return launch_generic(s3, plan, stream);
    }
    default:
      return launch_generic(r, plan, stream);
  }
}

}  // namespace flacenc_hip
