// frame_plan_test.cpp -- the plan of a frame-level call (flacenc_rs_amd/csrc/frame_plan.cpp) on the CPU.
//
// Links the real frame_plan.cpp and qlpc_dispatch.cpp, compiled for the host alone, against the stub launchers of
// stub_launchers.h and walks a grid of calls through plan_frame_call.  At every grid point:
//   1. the plan equals the conditions of the layer it replaced.  The legacy_* functions below are those conditions, copied
//      as they stood in the commit before plan_frame_call existed -- api_frames.cpp: frame_config and fixed_group_log2,
//      big_block_frames, the stereo call's and the Independent(n) call's path conditions; api_candidates.cpp: search_flags
//      and lpc_search, certify_needs_scratch, the two split-scratch conditions of the candidate batches -- with the handle
//      replaced by the two values read from it and the HIP calls by what they decided.  They are frozen: a change of
//      routing policy changes frame_plan.cpp and then this copy, on purpose.  The launch records the conditions read are
//      built by the shared field builders (config_record, frame_fields), which are verbatim moves of base_args and
//      frame_args and are NOT frozen here: how they derive reference_order, certify, integer_parity_only and force_generic
//      from the flags is held by tests/golden/dispatch_routes.txt's record fields and by the GPU suites, not by this test.
//   2. the plan is consistent with plan_qlpc_route: kFused routes to the fused kernel with the variant the call implies,
//      kBigBlock's analyse-only records route to the big-block kernels, kSubwave's record is eligible.
//   3. the scratch rule is sound: every record the plan launches goes through launch_qlpc with hipSuccess given what the
//      rule grants, and a launched record the rule denies the split scratch routes the same with the pointer set.
//
// The grid: calls x blocks x orders x row alignment x config switches x flags x handle state.  The full cross product of
// the flag bits is 481 M points, so the flag axis is thinned where a bit cannot matter: FUSED_PACK / TWO_STAGE_PACK vary
// only for the call with a pack target, INTEGER_PARITY_ONLY only beside REFERENCE / CANONICAL_SUM_ORDER, the handle's
// extra windows / precision floor only beside WINDOW_SEARCH / PRECISION_SEARCH, and the four search flags run as none, each
// alone and three combinations instead of all sixteen.  38 M points, a few seconds on eight threads.
//
//   frame_plan_test      prints "points N fused F bigblock B subwave S general G launches L" and exits 0, or the first
//                        failures and exits 1
#include <atomic>
#include <cstring>
#include <thread>

#include "stub_launchers.h"

#include "frame_plan.h"

namespace flacenc_hip {
namespace {

// the scratch a record was granted, as the predicates and plan_qlpc_route read it: addresses nothing dereferences
void grant_placeholders(QlpcKernelArgs& a, ScratchGrant g) {
  if (g.split) {
    a.split_scratch = reinterpret_cast<void*>(uintptr_t{0x20000000});
    a.marked_count = reinterpret_cast<uint32_t*>(uintptr_t{0x70000000});
  }
  if (g.sumabs) a.sumabs_scratch = reinterpret_cast<float*>(uintptr_t{0x60000000});
}

// ---- the parent's conditions ----------------------------------------------------------------------------------------

bool legacy_lpc_search(uint32_t flags) {
  return (flags & (FLACENC_HIP_FLAG_ORDER_SEARCH | FLACENC_HIP_FLAG_WINDOW_SEARCH | FLACENC_HIP_FLAG_ORDER_GUESS |
                   FLACENC_HIP_FLAG_PRECISION_SEARCH)) != 0;
}

uint32_t legacy_search_flags(bool windows_empty, uint32_t precision_floor, uint32_t flags, uint32_t quant_precision) {
  const uint32_t dropped =
      (((flags & FLACENC_HIP_FLAG_WINDOW_SEARCH) && windows_empty) ? FLACENC_HIP_FLAG_WINDOW_SEARCH : 0u) |
      (((flags & FLACENC_HIP_FLAG_PRECISION_SEARCH) && precision_floor >= quant_precision)
           ? FLACENC_HIP_FLAG_PRECISION_SEARCH : 0u);
  if (!dropped) return flags;
  flags &= ~dropped;
  if (legacy_lpc_search(flags)) return flags;
  flags &= ~(FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY);
  if (!(flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER)) flags |= FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER;
  return flags;
}

flacenc_hip_frame_config legacy_frame_config(bool windows_empty, uint32_t precision_floor, const flacenc_hip_frame_config* cfg,
                                             uint32_t block_size) {
  flacenc_hip_frame_config c = *cfg;
  c.qlpc.flags = legacy_search_flags(windows_empty, precision_floor, cfg->qlpc.flags, cfg->qlpc.quant_precision);
  if (block_size < FLACENC_HIP_MIN_BLOCK_SIZE) c.use_fixed = c.use_lpc = 0;
  return c;
}

uint32_t legacy_fixed_group_log2(const flacenc_hip_frame_config* cfg, bool* composite) {
  *composite = false;
  if (!cfg->use_fixed || cfg->fixed_order_sel != FLACENC_HIP_ORDERSEL_APPROXENT) return 0;
  const uint32_t p = cfg->fixed_partitions;
  *composite = (p & (p - 1)) != 0;
  uint32_t g = 0;
  for (uint32_t lanes = *composite ? 1u : 64u / p; lanes > 1; lanes >>= 1) ++g;
  return g;
}

bool legacy_big_block_frames(const flacenc_hip_frame_config* cfg, const QlpcKernelArgs& a) {
  const uint32_t block_size = a.block_size;
  const bool big_shape =
      cfg->use_lpc && (block_size == 8192 || block_size == 16384 || (block_size == 4096 && cfg->qlpc.lpc_order >= 13)) &&
      !(cfg->qlpc.flags & FLACENC_HIP_FLAG_GENERIC_KERNEL) && !cfg->qlpc.use_direct_mse &&
      (reinterpret_cast<uintptr_t>(a.samples) & 15) == 0 && (a.stride & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(a.residual) & 15) == 0 && (a.residual_stride & 3) == 0;
  const uint32_t fparts = cfg->fixed_partitions;
  const bool fixed_big = !cfg->use_fixed ||
                         (cfg->fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT && fparts != 0 && (fparts & (fparts - 1)) == 0 &&
                          block_size / fparts >= 64 && block_size / fparts <= 4096 && cfg->fixed_max_order <= 4);
  return big_shape && fixed_big;
}

bool legacy_certify_needs_scratch(const QlpcKernelArgs& a) {
  return a.certify != 0u && cert_shape(a) && (a.reference_order == 0u || a.integer_parity_only) &&
         !a.direct_mse && a.fixed_mode == 0 && (!wave_kernel_eligible(a) || a.pack_out != nullptr);
}

// api_candidates.cpp, enqueue_lpc: `a` the batch's record, `cfg` its (normalised) config
bool legacy_lpc_batch_split(const flacenc_hip_qlpc_config* cfg, const QlpcKernelArgs& a) {
  const uint32_t block_size = a.block_size;
  const bool order_search = legacy_lpc_search(cfg->flags);
  return cfg->lpc_order >= 13 || a.reference_order || a.direct_mse || block_size == 8192 || block_size == 16384 ||
         subwave_shape(block_size) || a.certify != 0u || order_search;
}

// api_candidates.cpp, enqueue_fixed under ApproxEnt (BitCount attached nothing)
bool legacy_fixed_batch_split(uint32_t block_size) {
  return block_size == 4096 || block_size == 8192 || block_size == 16384 || subwave_shape(block_size);
}

struct Legacy {
  flacenc_hip_frame_config cfg;
  int path;  // FramePlan::Path
  uint32_t group_log2, cert_subwave;
  bool packed, lpc_batch, fixed_batch;
  bool frame_record, frame_split, frame_sumabs, subwave_attach;
};

// the two entry points' bodies between their argument checks and their launches
Legacy legacy_call(const FrameCall& c) {
  Legacy L{};
  L.cfg = legacy_frame_config(!c.extra_windows, c.precision_floor, &c.cfg, c.block_size);
  const flacenc_hip_frame_config* cfg = &L.cfg;
  bool composite = false;
  L.group_log2 = legacy_fixed_group_log2(cfg, &composite);
  L.path = FramePlan::kGeneral;
  const bool order_search = (legacy_lpc_search(cfg->qlpc.flags) && cfg->use_lpc) || (cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE);
  QlpcKernelArgs a = config_record(cfg->qlpc, c.samples, c.stride, c.block_size, c.stereo ? 4 : 1, nullptr, c.bits_per_sample, c.stereo);
  a.residual = const_cast<int32_t*>(c.residual);
  a.residual_stride = c.residual_stride;
  frame_fields(a, *cfg, c.stereo, L.group_log2);
  const bool approx = cfg->use_fixed && cfg->fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT;
  auto attach_split = [&](QlpcKernelArgs& r) { grant_placeholders(r, {true, false}); };
  auto subwave = [&](bool frames) {
    QlpcKernelArgs m = a;
    m.stamps = nullptr;
    m.fixed_partitions = cfg->fixed_partitions;
    m.cert_subwave = (a.certify != 0u && a.reference_order == 0u && !a.direct_mse && cfg->use_lpc && cfg->qlpc.lpc_order <= 12) ? 1u : 0u;
    L.cert_subwave = m.cert_subwave;
    attach_split(m);
    L.subwave_attach = true;
    m.marked_unit = frames ? 4 : 1;
    return frames ? subwave_frame_eligible(m) : subwave_channels_eligible(m);
  };
  if (c.stereo) {
    L.frame_record = true;
    a.frame_results = reinterpret_cast<flacenc_hip_stereo_frame_result*>(uintptr_t{0xC0000000});
    if (a.reference_order) {  // R[] of the reference-order pass
      attach_split(a);
      L.frame_split = true;
      L.frame_sumabs = a.use_fixed && a.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT;
    }
    bool want_fused = false;
    if (cfg->qlpc.flags & FLACENC_HIP_FLAG_FUSED_PACK) want_fused = true;
    if (cfg->qlpc.flags & FLACENC_HIP_FLAG_TWO_STAGE_PACK) want_fused = false;
    if (c.pack && want_fused && !composite && !order_search && c.block_size == 4096 && wave_kernel_eligible(a)) {
      a.pack_out = reinterpret_cast<uint8_t*>(uintptr_t{0xD0000000});
      L.packed = true;
    }
    if (a.split_scratch == nullptr && legacy_certify_needs_scratch(a)) {
      attach_split(a);
      L.frame_split = true;
    }
    if (wave_kernel_eligible(a) && !composite && !order_search) L.path = FramePlan::kFused;
    else if (!order_search && legacy_big_block_frames(cfg, a)) L.path = FramePlan::kBigBlock;
    else if (c.block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && subwave_shape(c.block_size) && !order_search && subwave(true))
      L.path = FramePlan::kSubwave;
  } else if (!order_search) {
    L.frame_record = true;
    a.chan_results = reinterpret_cast<flacenc_hip_channel_result*>(uintptr_t{0xC4000000});
    if (a.reference_order || legacy_certify_needs_scratch(a)) {
      attach_split(a);
      L.frame_split = true;
    }
    L.frame_sumabs = a.reference_order && approx;
    if (!composite && wave_kernel_eligible(a)) L.path = FramePlan::kFused;
    else if (c.block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && subwave_shape(c.block_size) && subwave(false))
      L.path = FramePlan::kSubwave;
  }
  L.lpc_batch = L.path != FramePlan::kFused && cfg->use_lpc;
  L.fixed_batch = L.path != FramePlan::kFused && cfg->use_fixed;
  return L;
}

// ---- the grid -------------------------------------------------------------------------------------------------------

template <typename T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

struct CallKind { const char* name; bool stereo, pack; uint32_t channels; };
constexpr CallKind kCalls[] = {{"stereo", true, false, 2}, {"stereo_pack", true, true, 2}, {"independent1", false, false, 1},
                               {"independent3", false, false, 3}, {"independent8", false, false, 8}};
constexpr uint32_t kBlocks[] = {16, 63, 64, 192, 256, 288, 1152, 2304, 4096, 4608, 8192, 16384, 16400, 32767};
constexpr uint32_t kOrders[] = {1, 8, 10, 12, 13, 16, 32};
constexpr uint32_t kSelPartitions[] = {0, 1, 3, 32, 64};  // 0: BitCount
constexpr uint32_t kSumOrders[] = {0, FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER,
                                   FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY,
                                   FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER, FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER,
                                   FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY};
constexpr uint32_t kSearches[] = {0, FLACENC_HIP_FLAG_ORDER_SEARCH, FLACENC_HIP_FLAG_WINDOW_SEARCH, FLACENC_HIP_FLAG_ORDER_GUESS,
                                  FLACENC_HIP_FLAG_PRECISION_SEARCH, FLACENC_HIP_FLAG_WINDOW_SEARCH | FLACENC_HIP_FLAG_PRECISION_SEARCH,
                                  FLACENC_HIP_FLAG_ORDER_SEARCH | FLACENC_HIP_FLAG_WINDOW_SEARCH | FLACENC_HIP_FLAG_PRECISION_SEARCH,
                                  FLACENC_HIP_FLAG_ORDER_GUESS | FLACENC_HIP_FLAG_WINDOW_SEARCH};
constexpr uint32_t kPackFlags[] = {0, FLACENC_HIP_FLAG_FUSED_PACK, FLACENC_HIP_FLAG_TWO_STAGE_PACK,
                                   FLACENC_HIP_FLAG_FUSED_PACK | FLACENC_HIP_FLAG_TWO_STAGE_PACK};
constexpr uint32_t kQuantPrecision = 15;

struct Counts {
  uint64_t points = 0, path[4] = {0, 0, 0, 0}, launches = 0, failures = 0;
};
std::atomic<int> g_printed{0};

struct Checker {
  Counts n;
  Trace trace;
  const FrameCall* call = nullptr;
  const char* call_name = "";
  uint32_t channels = 0;

  void fail(const char* what) {
    ++n.failures;
    if (g_printed.fetch_add(1) >= 10) return;
    const FrameCall& c = *call;
    fprintf(stderr, "FAIL %s: %s block %u order %u samples %p rstride %zu use_lpc %u use_fixed %u sel %u parts %u mse %u flags 0x%x "
            "windows %d floor %u\n", what, call_name, c.block_size, c.cfg.qlpc.lpc_order, (const void*)c.samples, c.residual_stride,
            c.cfg.use_lpc, c.cfg.use_fixed, c.cfg.fixed_order_sel, c.cfg.fixed_partitions, c.cfg.qlpc.use_direct_mse,
            c.cfg.qlpc.flags, (int)c.extra_windows, c.precision_floor);
  }
  void expect(bool ok, const char* what) { if (!ok) fail(what); }

  static bool same_route(const QlpcRoute& x, const QlpcRoute& y) {
    return x.order == y.order && x.certify == y.certify && x.reference_order == y.reference_order && x.sumabs == y.sumabs &&
           x.direct_mse == y.direct_mse && x.chains_marked == y.chains_marked && x.chains_all == y.chains_all &&
           x.bigblock_acorr == y.bigblock_acorr && x.family == y.family && x.bucket == y.bucket && x.variant == y.variant &&
           x.bigblock == y.bigblock && x.cleanup == y.cleanup;
  }
  // a record the plan launches, with what the rule granted it: through the stubs, and (split denied) the same route with one
  void launched(const QlpcKernelArgs& rec, bool split_granted, bool subwave_frames_launcher, const char* what) {
    trace.hash = 0;
    trace.seq.clear();
    const QlpcLaunchPlan lp = plan_qlpc_launch(rec.block_size, rec.lpc_order);
    const hipError_t err = subwave_frames_launcher ? launch_subwave_frames(rec, kStream) : launch_qlpc(rec, lp, kStream);
    ++n.launches;
    expect(err == hipSuccess && !trace.seq.empty(), what);
    if (!split_granted) {
      QlpcKernelArgs with = rec;
      grant_placeholders(with, {true, false});
      expect(same_route(plan_qlpc_route(rec), plan_qlpc_route(with)), "a record denied the split scratch routes differently with one");
    }
  }

  void point(const FrameCall& c) {
    call = &c;
    ++n.points;
    const FramePlan p = plan_frame_call(c);
    const Legacy L = legacy_call(c);
    ++n.path[p.path];
    // 1. equals the parent
    expect(std::memcmp(&p.cfg, &L.cfg, sizeof p.cfg) == 0, "normalised config");
    expect(p.path == L.path, "path");
    expect(p.lpc_batch == L.lpc_batch && p.fixed_batch == L.fixed_batch, "candidate batches");
    expect(p.group_log2 == L.group_log2, "group_log2");
    expect(p.cert_subwave == L.cert_subwave, "cert_subwave");
    expect(p.fused_pack == L.packed, "fused pack");
    expect(p.frame_record == L.frame_record && p.subwave_scratch == L.subwave_attach, "records built");
    QlpcKernelArgs fr = probe_record(c, p, LaunchKind::kFrame);
    const ScratchGrant fg = p.frame_record ? scratch_grant(fr, LaunchKind::kFrame) : ScratchGrant{false, false};
    expect(fg.split == L.frame_split && fg.sumabs == L.frame_sumabs, "frame record's scratch");
    const QlpcKernelArgs lpc = probe_record(c, p, LaunchKind::kLpcBatch), fixed = probe_record(c, p, LaunchKind::kFixedBatch);
    const ScratchGrant lg = scratch_grant(lpc, LaunchKind::kLpcBatch, lpc_search(p.cfg.qlpc.flags));
    const ScratchGrant xg = scratch_grant(fixed, LaunchKind::kFixedBatch);
    const bool approx = p.cfg.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT;
    expect(lg.split == legacy_lpc_batch_split(&p.cfg.qlpc, lpc) && !lg.sumabs, "LPC batch's scratch");
    expect(xg.split == (approx && legacy_fixed_batch_split(c.block_size)) && xg.sumabs == (approx && fixed.reference_order != 0u),
           "fixed batch's scratch");
    // 2. consistent with the route planner, 3. the scratch rule is sound
    grant_placeholders(fr, fg);
    fr.n_subframes = c.stereo ? 8 : 2 * channels;
    if (p.path == FramePlan::kFused) {
      const QlpcRoute rt = plan_qlpc_route(fr);
      const int v = c.stereo ? (p.fused_pack ? 5 : (p.cfg.use_fixed ? 3 : 2)) : 4;
      expect(rt.family == QlpcRoute::kFused && (rt.variant == v || ((v == 3 || v == 4) && rt.variant == v + 3)), "kFused: route");
      launched(fr, fg.split, false, "kFused: launch");
      return;
    }
    auto batches = [&](bool analyse_only) {
      if (p.lpc_batch && !lpc_search(p.cfg.qlpc.flags)) {  // (a search's record goes to launch_order_search)
        QlpcKernelArgs r = lpc;
        grant_placeholders(r, lg);
        r.params = fake<flacenc_hip_subframe_params>(0x50000000);
        r.n_subframes = fr.n_subframes;
        if (analyse_only) r.residual_mode = 1u, r.minmax_out = fake<int32_t>(0x98000000);
        const QlpcRoute rt = plan_qlpc_route(r);
        if (analyse_only) expect(rt.family == QlpcRoute::kBigBlock && rt.bigblock, "kBigBlock: QLPC record's route");
        launched(r, lg.split, false, "LPC batch: launch");
      }
      if (p.fixed_batch) {
        QlpcKernelArgs r = fixed;
        grant_placeholders(r, xg);
        r.params = fake<flacenc_hip_subframe_params>(0x50000000);
        r.n_subframes = fr.n_subframes;
        r.selector_keys = fake<unsigned long long>(0xE0000000);
        if (analyse_only) {
          r.residual_mode = 1u;
          expect(plan_qlpc_route(r).family == QlpcRoute::kBigBlockFixed, "kBigBlock: fixed record's route");
        }
        if (r.fixed_mode == 0) {  // BitCount: every order, then the chosen ones
          r.fixed_mode = 2;
          launched(r, xg.split, false, "fixed batch (BitCount, mode 2): launch");
          r.fixed_mode = 3;
          r.forced_orders = fake<const uint8_t>(0xE8000000);
        }
        launched(r, xg.split, false, "fixed batch: launch");
      }
    };
    if (p.path == FramePlan::kBigBlock) {
      expect(!p.search_or_escape, "kBigBlock: analyse-only batches under a search flag or RICE_ESCAPE");
      batches(true);
      return;
    }
    if (p.path == FramePlan::kSubwave) {
      QlpcKernelArgs m = fr;
      subwave_fields(m, p.cfg, p.cert_subwave);
      grant_placeholders(m, scratch_grant(m, LaunchKind::kSubwaveFrames));
      m.marked_unit = c.stereo ? 4 : 1;
      expect(c.stereo ? subwave_frame_eligible(m) : subwave_channels_eligible(m), "kSubwave: eligibility");
      m.cand_lpc_params = fake<const flacenc_hip_subframe_params>(0x51000000);
      if (p.cfg.use_fixed) m.cand_fixed_params = fake<const flacenc_hip_subframe_params>(0x52000000);
      launched(m, true, true, "kSubwave: launch");
      QlpcKernelArgs cl = m;  // the clean-ups (subwave_frames, api_frames.cpp)
      cl.frame_results = nullptr;
      cl.chan_results = nullptr;
      cl.cand_lpc_params = cl.cand_fixed_params = nullptr;
      cl.params = fake<flacenc_hip_subframe_params>(0x50000000);
      cl.residual = lpc.residual;
      cl.residual_stride = lpc.residual_stride;
      cl.only_marked = 1;
      cl.use_fixed = 0;
      launched(cl, true, false, "kSubwave: QLPC clean-up");
      if (p.cfg.use_fixed) {
        cl.selector_keys = fake<unsigned long long>(0xE0000000);
        fixed_batch_fields(cl, p.cfg);
        launched(cl, true, false, "kSubwave: fixed clean-up");
      }
      return;
    }
    batches(false);
  }
};

void run_group(int call_index, uint32_t block, Checker& ck) {
  const CallKind& kind = kCalls[call_index];
  ck.call_name = kind.name;
  ck.channels = kind.channels;
  FrameCall c{};
  c.stereo = kind.stereo;
  c.pack = kind.pack;
  c.block_size = block;
  c.bits_per_sample = 16;
  const size_t pstride = padded_stride(block);
  for (uint32_t order : kOrders)
    for (int align = 0; align < 3; ++align) {
      c.samples = fake<const int32_t>(align == 1 ? 0x10000004 : 0x10000000);  // 1: rows off by 4 bytes
      c.stride = pstride;
      c.residual = fake<const int32_t>(0x40000000);
      c.residual_stride = align == 2 ? (pstride | 1) : pstride;                // 2: an odd residual stride
      for (int sw = 0; sw < 8; ++sw)
        for (uint32_t parts : kSelPartitions) {
          c.cfg = flacenc_hip_frame_config{};
          c.cfg.use_constant = 1;
          c.cfg.use_leftside = c.cfg.use_rightside = c.cfg.use_midside = 1;
          c.cfg.use_lpc = sw & 1;
          c.cfg.use_fixed = (sw >> 1) & 1;
          c.cfg.qlpc.use_direct_mse = (sw >> 2) & 1;
          c.cfg.fixed_max_order = 4;
          c.cfg.fixed_order_sel = parts ? FLACENC_HIP_ORDERSEL_APPROXENT : FLACENC_HIP_ORDERSEL_BITCOUNT;
          c.cfg.fixed_partitions = parts;
          c.cfg.qlpc.lpc_order = order;
          c.cfg.qlpc.quant_precision = kQuantPrecision;
          c.cfg.qlpc.max_rice_parameter = 14;
          for (uint32_t generic : {0u, (uint32_t)FLACENC_HIP_FLAG_GENERIC_KERNEL})
            for (uint32_t pack_flags : kPackFlags) {
              if (pack_flags && !kind.pack) continue;
              for (uint32_t sum : kSumOrders)
                for (uint32_t search : kSearches)
                  for (uint32_t escape : {0u, (uint32_t)FLACENC_HIP_FLAG_RICE_ESCAPE}) {
                    c.cfg.qlpc.flags = generic | pack_flags | sum | search | escape;
                    const int windows = (search & FLACENC_HIP_FLAG_WINDOW_SEARCH) ? 2 : 1;
                    const int floors = (search & FLACENC_HIP_FLAG_PRECISION_SEARCH) ? 2 : 1;
                    for (int w = 0; w < windows; ++w)
                      for (int f = 0; f < floors; ++f) {
                        c.extra_windows = w == 0;
                        c.precision_floor = f == 0 ? 5 : kQuantPrecision;  // below / at quant_precision
                        ck.point(c);
                      }
                  }
            }
        }
    }
}

}  // namespace
}  // namespace flacenc_hip

int main() {
  using namespace flacenc_hip;
  register_launchers();
  constexpr int kNumCalls = static_cast<int>(sizeof kCalls / sizeof kCalls[0]);
  constexpr int kNumBlocks = static_cast<int>(sizeof kBlocks / sizeof kBlocks[0]);
  unsigned n_threads = std::thread::hardware_concurrency();
  n_threads = n_threads < 1 ? 1 : (n_threads > 8 ? 8 : n_threads);
  std::vector<Checker> checkers(n_threads);
  std::atomic<int> next{0};
  std::vector<std::thread> workers;
  for (unsigned w = 0; w < n_threads; ++w)
    workers.emplace_back([&, w] {
      g_trace = &checkers[w].trace;
      for (int i; (i = next.fetch_add(1)) < kNumCalls * kNumBlocks;) run_group(i / kNumBlocks, kBlocks[i % kNumBlocks], checkers[w]);
    });
  for (std::thread& w : workers) w.join();
  Counts t;
  for (const Checker& ck : checkers) {
    t.points += ck.n.points;
    t.launches += ck.n.launches;
    t.failures += ck.n.failures;
    for (int i = 0; i < 4; ++i) t.path[i] += ck.n.path[i];
  }
  printf("points %" PRIu64 " fused %" PRIu64 " bigblock %" PRIu64 " subwave %" PRIu64 " general %" PRIu64 " launches %" PRIu64
         " failures %" PRIu64 "\n", t.points, t.path[FramePlan::kFused], t.path[FramePlan::kBigBlock], t.path[FramePlan::kSubwave],
         t.path[FramePlan::kGeneral], t.launches, t.failures);
  return t.failures ? 1 : 0;
}
