// stub_launchers.h -- the launchers flacenc_rs_amd/csrc/qlpc_dispatch.cpp calls, as stubs for host programs that link the
// real dispatch unit without a device (dispatch_trace.cpp, frame_plan_test.cpp): a stub makes no HIP call, it appends its
// own name and every field of the record it was given to the thread's trace (g_trace, which the program sets) and
// returns hipSuccess.  Included by exactly one translation unit of a program.
#ifndef FLACENC_HIP_TESTS_STUB_LAUNCHERS_H_
#define FLACENC_HIP_TESTS_STUB_LAUNCHERS_H_

#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "qlpc_kernel.h"

#include "acorr_reference.h"
#include "direct_mse.h"
#include "sumabs_reference.h"

namespace flacenc_hip {
namespace {

// ---- the trace ------------------------------------------------------------------------------------------------------

struct Trace {
  uint64_t hash = 0;
  std::vector<uint16_t> seq;  // launcher ids in call order
  std::string* text = nullptr;  // --dump: the lines themselves
};
thread_local Trace* g_trace = nullptr;

inline uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  h *= 0xFF51AFD7ED558CCDull;
  return h ^ (h >> 29);
}

std::vector<std::string>& launcher_names() {
  static std::vector<std::string> names;
  return names;
}
// (called from main for every stub before the grid runs: ids are the table's order, not the order of first use)
int launcher_id(const char* name) {
  std::vector<std::string>& names = launcher_names();
  for (size_t i = 0; i < names.size(); ++i)
    if (names[i] == name) return static_cast<int>(i);
  names.emplace_back(name);
  return static_cast<int>(names.size()) - 1;
}

struct Field {
  void operator()(const char* name, uint64_t v) const {
    g_trace->hash = mix(g_trace->hash, v);
    if (g_trace->text) {
      char buf[96];
      snprintf(buf, sizeof buf, " %s=0x%" PRIx64, name, v);
      *g_trace->text += buf;
    }
  }
  template <typename T>
  void operator()(const char* name, T* p) const { (*this)(name, static_cast<uint64_t>(reinterpret_cast<uintptr_t>(p))); }
  void operator()(const char* name, int32_t v) const { (*this)(name, static_cast<uint64_t>(static_cast<int64_t>(v))); }
  void operator()(const char* name, uint32_t v) const { (*this)(name, static_cast<uint64_t>(v)); }
};

#define F(x) f(#x, a.x);
void fields(const QlpcKernelArgs& a) {
  // every member, in declaration order; a new member changes the size and must be added here
  static_assert(sizeof(QlpcKernelArgs) == 608, "QlpcKernelArgs changed: list the new member below");
  const Field f;
  F(samples) F(stride) F(block_size) F(n_subframes) F(bps) F(bps_uniform) F(stereo) F(window) F(window_lanes) F(flat_lo)
  F(flat_hi) F(lpc_order) F(precision) F(max_rice_parameter) F(rice_finest_only) F(force_generic) F(reference_order)
  F(acorr_in) F(certify) F(cert_subwave) F(acorr_marked) F(integer_parity_only) F(cert_stats) F(sumabs_in)
  F(sumabs_scratch) F(sumabs_mode) F(direct_mse) F(mae_steps) F(direct_mse_scratch) F(irls_weight_scratch) F(residual_lr)
  F(residual_lr_stride) F(minmax_out) F(residual_mode) F(cand_lpc_params) F(cand_fixed_params) F(cand_fixed_keys)
  F(cand_minmax) F(cand_lpc_rows) F(cand_fixed_rows) F(cand_stride) F(only_marked) F(marked_count) F(marked_next)
  F(marked_list) F(marked_cap) F(marked_unit) F(params) F(residual) F(residual_stride) F(autocorr) F(lpc_coefs)
  F(table_scratch) F(stamps) F(frame_results) F(chan_results) F(use_constant) F(use_lpc) F(use_leftside) F(use_rightside)
  F(use_midside) F(use_fixed) F(fixed_max_order) F(fixed_order_sel) F(fixed_group_log2) F(fixed_keys) F(fixed_mode)
  F(fixed_partitions) F(forced_uniform) F(forced_orders) F(selector_keys) F(lpc_stage) F(pred) F(pred_out) F(split_scratch)
  F(pack_out) F(pack_out_stride) F(pack_out_len) F(pack_header_mid) F(pack_extra_len) F(pack_first_frame)
  F(pack_frame_step) F(pack_lds_words) F(pack_crc_per)
  uint64_t extra = 0, pow = 0;
  for (int i = 0; i < 4; ++i) extra = extra << 8 | a.pack_extra[i];
  for (int i = 0; i < 32; ++i) pow = mix(pow, a.pack_crc_pow[i]);
  f("pack_extra", extra);
  f("pack_crc_pow#", pow);
}
void fields(const AcorrRefArgs& a) {
  const Field f;
  F(samples) F(stride) F(block_size) F(n_subframes) F(stereo) F(window) F(lpc_order) F(nightly) F(out) F(out_stride)
  F(marked_params) F(marked_count) F(marked_list) F(marked_cap) F(marked_unit)
}
void fields(const SumAbsRefArgs& a) {
  const Field f;
  F(samples) F(stride) F(block_size) F(n_subframes) F(stereo) F(partitions) F(nightly) F(out)
}
void fields(const DirectMseArgs& a) {
  const Field f;
  F(samples) F(stride) F(block_size) F(n_subframes) F(stereo) F(window) F(lpc_order) F(precision) F(mae_steps) F(pred_out)
  F(autocorr) F(lpc_coefs) F(weight_scratch) F(gram_scratch) F(irls_state) F(irls_weights) F(irls_step)
}
#undef F

hipStream_t const kStream = reinterpret_cast<hipStream_t>(uintptr_t{0x7770000});

template <typename Args>
hipError_t emit(int id, const Args& a, hipStream_t stream, int threads = -1, size_t smem = 0) {
  Trace& t = *g_trace;
  t.seq.push_back(static_cast<uint16_t>(id));
  t.hash = mix(t.hash, 0x1000u + static_cast<uint64_t>(id));
  if (t.text) *t.text += "  " + launcher_names()[id];
  fields(a);
  const Field f;
  if (threads >= 0) {
    f("threads", static_cast<uint64_t>(threads));
    f("smem", static_cast<uint64_t>(smem));
  }
  f("stream", stream);
  if (t.text) *t.text += "\n";
  return hipSuccess;
}

}  // namespace

// ---- the stub launchers: every launcher the dispatch unit calls -----------------------------------------------------

#define STUB_BODY(NAME, ...)                              \
  {                                                       \
    static const int id = launcher_id(NAME);              \
    return emit(id, a, __VA_ARGS__);                      \
  }
#define STUB_INSTANCE(MP, BG)                                                                                   \
  hipError_t launch_qlpc_##MP##_##BG(const QlpcKernelArgs& a, int threads, size_t smem, hipStream_t s)          \
      STUB_BODY("launch_qlpc_" #MP "_" #BG, s, threads, smem)                                                   \
  hipError_t launch_levinson_##MP##_##BG(const QlpcKernelArgs& a, hipStream_t s) STUB_BODY("launch_levinson_" #MP "_" #BG, s)
FLACENC_HIP_FOR_EACH_INSTANCE(STUB_INSTANCE)
#define STUB_WAVE(MP, ST) \
  hipError_t launch_qlpc_wave_##MP##_##ST(const QlpcKernelArgs& a, hipStream_t s) STUB_BODY("launch_qlpc_wave_" #MP "_" #ST, s)
FLACENC_HIP_FOR_EACH_WAVE_INSTANCE(STUB_WAVE)
#define STUB_WAVE72(MP, ST) \
  hipError_t launch_qlpc_wave72_##MP##_##ST(const QlpcKernelArgs& a, hipStream_t s) STUB_BODY("launch_qlpc_wave72_" #MP "_" #ST, s)
FLACENC_HIP_FOR_EACH_WAVE72_INSTANCE(STUB_WAVE72)
#define STUB_SUBWAVE(MP, ST, SP, V)                                                              \
  hipError_t launch_qlpc_subwave_##MP##_##ST##_##SP##_##V(const QlpcKernelArgs& a, hipStream_t s) \
      STUB_BODY("launch_qlpc_subwave_" #MP "_" #ST "_" #SP "_" #V, s)
FLACENC_HIP_FOR_EACH_SUBWAVE_INSTANCE(STUB_SUBWAVE)
#define STUB_PLAIN(NAME, ARGS) hipError_t NAME(const ARGS& a, hipStream_t s) STUB_BODY(#NAME, s)
STUB_PLAIN(launch_bigblock_acorr, QlpcKernelArgs)
STUB_PLAIN(launch_bigblock_residual, QlpcKernelArgs)
STUB_PLAIN(launch_bigblock_fixed_select, QlpcKernelArgs)
STUB_PLAIN(launch_bigblock_fixed_residual, QlpcKernelArgs)
STUB_PLAIN(launch_acorr_reference, AcorrRefArgs)
STUB_PLAIN(launch_sumabs_reference, SumAbsRefArgs)
STUB_PLAIN(launch_direct_mse, DirectMseArgs)

namespace {

// the table of launcher names, in the order of the lists above (a stub that is never called still has its row)
void register_launchers() {
#define REG_INSTANCE(MP, BG) launcher_id("launch_qlpc_" #MP "_" #BG); launcher_id("launch_levinson_" #MP "_" #BG);
  FLACENC_HIP_FOR_EACH_INSTANCE(REG_INSTANCE)
#define REG_WAVE(MP, ST) launcher_id("launch_qlpc_wave_" #MP "_" #ST);
  FLACENC_HIP_FOR_EACH_WAVE_INSTANCE(REG_WAVE)
#define REG_WAVE72(MP, ST) launcher_id("launch_qlpc_wave72_" #MP "_" #ST);
  FLACENC_HIP_FOR_EACH_WAVE72_INSTANCE(REG_WAVE72)
#define REG_SUBWAVE(MP, ST, SP, V) launcher_id("launch_qlpc_subwave_" #MP "_" #ST "_" #SP "_" #V);
  FLACENC_HIP_FOR_EACH_SUBWAVE_INSTANCE(REG_SUBWAVE)
  for (const char* n : {"launch_bigblock_acorr", "launch_bigblock_residual", "launch_bigblock_fixed_select",
                        "launch_bigblock_fixed_residual", "launch_acorr_reference", "launch_sumabs_reference",
                        "launch_direct_mse"})
    launcher_id(n);
}

}  // namespace
}  // namespace flacenc_hip
#endif
