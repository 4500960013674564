// dispatch_trace.cpp -- characterisation of the launch routing (flacenc_rs_amd/csrc/qlpc_dispatch.cpp) on the CPU.
//
// The real dispatch unit, compiled for the host alone, is linked against the stub launchers of stub_launchers.h: a stub
// makes no HIP call, it appends its own name and every field of the record it was given to the trace.  The program walks a grid of
// launch records through launch_qlpc (and launch_subwave_frames) and prints, per (call shape, block size, order) group,
// the number of cases, a 64-bit hash over the group's full traces and the number of distinct launcher sequences; then
// every distinct launcher sequence of the whole grid with its count, and every launcher with the number of calls.
//
//   dispatch_trace                 the digests (what tests/golden/dispatch_routes.txt holds)
//   dispatch_trace --record FILE   the same, written to FILE
//   dispatch_trace --dump SHAPE:BLOCK:ORDER   the group's full traces, one line per launch (to diff two builds)
//
// Pointers are fixed fake addresses that nothing dereferences, so a derived pointer shows as what it is.
#include <algorithm>
#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "stub_launchers.h"

#include "frame_plan.h"

namespace flacenc_hip {
namespace {

// ---- the grid -------------------------------------------------------------------------------------------------------

template <typename T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

constexpr uint32_t kBlocks[] = {64, 192, 256, 288, 1152, 2048, 2304, 4096, 4608, 8192, 16384, 16400, 32768};
constexpr uint32_t kOrders[] = {1, 8, 9, 10, 12, 13, 16, 17, 24, 32};

struct Shape {
  const char* name;
  bool fixed_batch;     // runs at order 4 only, as enqueue_fixed sets it
  bool subwave_frames;  // through launch_subwave_frames instead of launch_qlpc
  void (*fill)(QlpcKernelArgs&);
};

// what every launch starts from: the real config_record (frame_plan.cpp) of an unflagged config -- the flag-derived words
// are the axes' (apply_axes) --, then what base_args and the callers (api_candidates.cpp) add
QlpcKernelArgs base_record(uint32_t block, uint32_t order, const QlpcLaunchPlan& plan) {
  flacenc_hip_qlpc_config q{};
  q.lpc_order = order;
  q.quant_precision = 15;
  q.max_rice_parameter = 14;
  QlpcKernelArgs a = config_record(q, fake<const int32_t>(0x10000000), padded_stride(block), block, 7, nullptr, 16, false);
  a.window = fake<const float>(0x30000000);
  a.window_lanes = block == 4096 ? fake<const float>(0x31000000) : nullptr;
  a.flat_lo = static_cast<int32_t>(block / 4);
  a.flat_hi = static_cast<int32_t>(block - block / 4);
  a.params = fake<flacenc_hip_subframe_params>(0x50000000);
  a.residual = fake<int32_t>(0x40000000);
  a.residual_stride = a.stride;
  a.marked_next = fake<uint32_t>(0x70000004);
  a.marked_list = fake<uint32_t>(0x70000040);
  a.marked_cap = 1024;
  a.table_scratch = plan.table_scratch_bytes_per_subframe ? fake<uint32_t>(0xB0000000) : nullptr;
  return a;
}

void stereo(QlpcKernelArgs& a, uint32_t n) {
  a.stereo = 1;
  a.n_subframes = n;
}
// frame_fields (frame_plan.cpp) + run_frame_plan (api_frames.cpp): results, no records
void frame_decision(QlpcKernelArgs& a, uint32_t use_fixed, uint32_t sel) {
  stereo(a, 8);
  a.params = nullptr;
  a.frame_results = fake<flacenc_hip_stereo_frame_result>(0xC0000000);
  a.stamps = fake<unsigned long long>(0xC8000000);
  a.use_fixed = use_fixed;
  a.fixed_max_order = 4;
  a.fixed_order_sel = sel;
  a.fixed_group_log2 = (use_fixed && sel) ? 2 : 0;  // 16 estimator partitions
}
void packed(QlpcKernelArgs& a) {
  a.pack_out = fake<uint8_t>(0xD0000000);
  a.pack_out_stride = 16384 + 64;
  a.pack_out_len = fake<uint32_t>(0xD8000000);
  a.pack_header_mid = 0xC918;
  a.pack_extra_len = 2;
  a.pack_extra[0] = 0x0F;
  a.pack_extra[1] = 0xFF;
  a.pack_frame_step = 1;
  a.pack_lds_words = 3072;
  a.pack_crc_per = 96;
  for (int i = 0; i < 32; ++i) a.pack_crc_pow[i] = static_cast<uint16_t>(0x8005u + 37u * i);
}
// enqueue_fixed (api_candidates.cpp)
void fixed_batch(QlpcKernelArgs& a, uint32_t mode, uint32_t partitions) {
  a.window = nullptr;
  a.window_lanes = nullptr;
  a.flat_lo = a.flat_hi = 0;
  a.precision = 0;
  a.use_fixed = 1;
  a.fixed_max_order = 4;
  a.fixed_order_sel = mode == 1 ? 1 : 0;
  a.fixed_partitions = partitions;
  a.fixed_mode = mode;
  a.selector_keys = mode == 3 ? nullptr : fake<unsigned long long>(0xE0000000);
  if (mode == 2) a.forced_uniform = 3;
  if (mode == 3) a.forced_orders = fake<const uint8_t>(0xE8000000);
}
// the QLPC clean-up behind the sub-wave frame kernels (subwave_frames, api_frames.cpp)
void cleanup(QlpcKernelArgs& a, uint32_t cert_subwave, bool acorr_marked) {
  stereo(a, 8);
  a.only_marked = 1;
  a.marked_unit = 4;
  a.cert_subwave = cert_subwave;
  a.fixed_max_order = 4;
  a.fixed_order_sel = 1;
  a.fixed_partitions = 4;
  if (acorr_marked) a.acorr_marked = fake<const double>(0x20000000);
}
void direct_mse(QlpcKernelArgs& a, uint32_t mae_steps) {
  a.direct_mse = 1;
  a.mae_steps = mae_steps;
  a.direct_mse_scratch = fake<double>(0xF0000000);
  if (mae_steps) a.irls_weight_scratch = fake<float>(0xF8000000);
}
// subwave_frames (api_frames.cpp): the record launch_subwave_frames is given
void subwave_frames(QlpcKernelArgs& a, bool frames, uint32_t cert_subwave, bool acorr_in) {
  if (frames) {
    frame_decision(a, 1, 1);
    a.marked_unit = 4;
  } else {
    a.n_subframes = 6;
    a.params = nullptr;
    a.chan_results = fake<flacenc_hip_channel_result>(0xC4000000);
    a.use_leftside = a.use_rightside = a.use_midside = 0;
    a.use_fixed = 1;
    a.fixed_max_order = 4;
    a.fixed_order_sel = 1;
  }
  a.stamps = nullptr;
  a.fixed_partitions = 4;
  a.cert_subwave = cert_subwave;
  a.cand_lpc_params = fake<const flacenc_hip_subframe_params>(0x51000000);
  a.cand_fixed_params = fake<const flacenc_hip_subframe_params>(0x52000000);
  if (acorr_in) a.acorr_in = fake<const double>(0x88000000);
}

const Shape kShapes[] = {
    {"cand", false, false, [](QlpcKernelArgs&) {}},
    {"cand_stereo8", false, false, [](QlpcKernelArgs& a) { stereo(a, 8); }},
    {"cand_stereo6", false, false, [](QlpcKernelArgs& a) { stereo(a, 6); }},
    {"frame", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 0, 0); }},
    {"frame_fixed_bitcount", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 1, 0); }},
    {"frame_nofixed_approxent", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 0, 1); }},
    {"frame_fixed_approxent", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 1, 1); }},
    {"pack", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 0, 0); packed(a); }},
    {"pack_fixed_bitcount", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 1, 0); packed(a); }},
    {"pack_nofixed_approxent", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 0, 1); packed(a); }},
    {"pack_fixed_approxent", false, false, [](QlpcKernelArgs& a) { frame_decision(a, 1, 1); packed(a); }},
    {"channels", false, false,
     [](QlpcKernelArgs& a) {
       a.n_subframes = 6;
       a.params = nullptr;
       a.chan_results = fake<flacenc_hip_channel_result>(0xC4000000);
       a.use_leftside = a.use_rightside = a.use_midside = 0;
       a.use_fixed = 1;
       a.fixed_max_order = 4;
       a.fixed_order_sel = 1;
       a.fixed_group_log2 = 2;
     }},
    {"fixed1_p1", true, false, [](QlpcKernelArgs& a) { fixed_batch(a, 1, 1); }},
    {"fixed1_p3", true, false, [](QlpcKernelArgs& a) { fixed_batch(a, 1, 3); }},
    {"fixed1_p4", true, false, [](QlpcKernelArgs& a) { stereo(a, 8); fixed_batch(a, 1, 4); }},
    {"fixed1_p64", true, false, [](QlpcKernelArgs& a) { fixed_batch(a, 1, 64); }},
    {"fixed2", true, false, [](QlpcKernelArgs& a) { fixed_batch(a, 2, 0); }},
    {"fixed3", true, false, [](QlpcKernelArgs& a) { fixed_batch(a, 3, 0); }},
    {"cleanup", false, false, [](QlpcKernelArgs& a) { cleanup(a, 0, false); }},
    {"cleanup_cert", false, false, [](QlpcKernelArgs& a) { cleanup(a, 1, false); }},
    {"cleanup_marked", false, false, [](QlpcKernelArgs& a) { cleanup(a, 0, true); }},
    {"cleanup_cert_marked", false, false, [](QlpcKernelArgs& a) { cleanup(a, 1, true); }},
    {"direct_mse", false, false, [](QlpcKernelArgs& a) { direct_mse(a, 0); }},
    {"direct_mse_mae2", false, false, [](QlpcKernelArgs& a) { stereo(a, 8); direct_mse(a, 2); }},
    {"acorr_in", false, false, [](QlpcKernelArgs& a) { a.acorr_in = fake<const double>(0x88000000); }},
    {"analyse_only", false, false,
     [](QlpcKernelArgs& a) {
       stereo(a, 8);
       a.residual_mode = 1;
       a.minmax_out = fake<int32_t>(0x98000000);
     }},
    {"residual_lr", false, false,
     [](QlpcKernelArgs& a) {
       stereo(a, 8);
       a.residual_lr = fake<int32_t>(0x94000000);
       a.residual_lr_stride = a.stride;
       a.minmax_out = fake<int32_t>(0x98000000);
     }},
    {"sw_frames", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, true, 0, false); }},
    {"sw_frames_cert", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, true, 1, false); }},
    {"sw_frames_acorr", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, true, 0, true); }},
    {"sw_frames_cert_acorr", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, true, 1, true); }},
    {"sw_channels", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, false, 0, false); }},
    {"sw_channels_cert", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, false, 1, false); }},
    {"sw_channels_acorr", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, false, 0, true); }},
    {"sw_channels_cert_acorr", false, true, [](QlpcKernelArgs& a) { subwave_frames(a, false, 1, true); }},
};
constexpr int kNumShapes = static_cast<int>(sizeof kShapes / sizeof kShapes[0]);

// the flag axes, as digits of a mixed-radix case number (the full cross product)
struct Axis {
  const char* name;
  int values;
};
constexpr Axis kAxes[] = {{"certify", 2},       {"reference_order", 3}, {"integer_parity_only", 2}, {"split_scratch", 2},
                          {"sumabs_scratch", 2}, {"force_generic", 2},   {"alignment", 3},           {"bps", 3},
                          {"autocorr", 2},       {"marked_count", 2}};
constexpr int kNumAxes = static_cast<int>(sizeof kAxes / sizeof kAxes[0]);
constexpr int num_flag_cases() {
  int n = 1;
  for (const Axis& ax : kAxes) n *= ax.values;
  return n;
}
constexpr int kFlagCases = num_flag_cases();  // + one case with n_subframes == 0

void apply_axes(QlpcKernelArgs& a, int number) {
  int v[kNumAxes];
  for (int i = 0; i < kNumAxes; ++i) {
    v[i] = number % kAxes[i].values;
    number /= kAxes[i].values;
  }
  a.certify = static_cast<uint32_t>(v[0]);
  a.reference_order = static_cast<uint32_t>(v[1]);
  a.integer_parity_only = static_cast<uint32_t>(v[2]);
  a.split_scratch = v[3] ? fake<void>(0x20000000) : nullptr;
  a.sumabs_scratch = v[4] ? fake<float>(0x60000000) : nullptr;
  a.force_generic = static_cast<uint32_t>(v[5]);
  if (v[6] == 1) a.samples = fake<const int32_t>(0x10000004);  // rows off by 4 bytes
  if (v[6] == 2) a.residual_stride |= 1;                       // an odd row stride
  a.bps = v[7] == 2 ? fake<const uint8_t>(0xA0000000) : nullptr;
  a.bps_uniform = v[7] == 0 ? 16 : (v[7] == 1 ? 24 : 0);
  if (v[8]) {
    a.autocorr = fake<double>(0x80000000);
    a.lpc_coefs = fake<double>(0x90000000);
  }
  a.marked_count = v[9] ? fake<uint32_t>(0x70000000) : nullptr;
}

std::string describe_case(int number) {
  if (number == kFlagCases) return "n_subframes=0";
  std::string s;
  for (int i = 0; i < kNumAxes; ++i) {
    s += std::string(i ? " " : "") + kAxes[i].name + "=" + std::to_string(number % kAxes[i].values);
    number /= kAxes[i].values;
  }
  return s;
}

const char* error_name(int err) {
  switch (static_cast<hipError_t>(err)) {
    case hipSuccess: return "hipSuccess";
    case hipErrorInvalidValue: return "hipErrorInvalidValue";
    case hipErrorNotSupported: return "hipErrorNotSupported";
    default: return "hipError?";
  }
}

struct Group {
  int shape;
  uint32_t block, order;
  uint64_t hash = 0;
  uint32_t cases = 0, sequences = 0;
};

struct SequenceCount {
  std::vector<uint16_t> launchers;
  int ret = 0;
  uint64_t count = 0;
};
using SequenceTable = std::map<uint64_t, SequenceCount>;  // by the sequence's hash

void run_group(Group& g, SequenceTable& table, std::vector<uint64_t>& calls, std::string* dump) {
  const Shape& shape = kShapes[g.shape];
  const QlpcLaunchPlan plan = plan_qlpc_launch(g.block, g.order);
  std::map<uint64_t, int> seen;
  Trace t;
  t.text = dump;
  g_trace = &t;
  for (int c = 0; c <= kFlagCases; ++c) {
    QlpcKernelArgs a = base_record(g.block, g.order, plan);
    shape.fill(a);
    apply_axes(a, c == kFlagCases ? 0 : c);
    if (c == kFlagCases) a.n_subframes = 0;
    t.hash = 0;
    t.seq.clear();
    if (dump) *dump += "case " + std::to_string(c) + ": " + describe_case(c) + "\n";
    const hipError_t err = shape.subwave_frames ? launch_subwave_frames(a, kStream) : launch_qlpc(a, plan, kStream);
    if (dump) *dump += "  => " + std::string(error_name(err)) + "\n";
    g.hash = mix(mix(g.hash, t.hash), static_cast<uint64_t>(err));
    uint64_t sh = static_cast<uint64_t>(err);
    for (uint16_t id : t.seq) {
      sh = mix(sh, id);
      ++calls[id];
    }
    SequenceCount& sc = table[sh];
    if (sc.count++ == 0) {
      sc.launchers = t.seq;
      sc.ret = static_cast<int>(err);
    }
    ++seen[sh];
    ++g.cases;
  }
  g.sequences = static_cast<uint32_t>(seen.size());
  g_trace = nullptr;
}

std::vector<Group> make_groups() {
  std::vector<Group> groups;
  for (int s = 0; s < kNumShapes; ++s)
    for (uint32_t block : kBlocks) {
      if (kShapes[s].fixed_batch) {
        groups.push_back(Group{s, block, 4});
        continue;
      }
      for (uint32_t order : kOrders) groups.push_back(Group{s, block, order});
    }
  return groups;
}


int digests(FILE* out) {
  std::vector<Group> groups = make_groups();
  const size_t n_launchers = launcher_names().size();
  unsigned n_threads = std::thread::hardware_concurrency();
  n_threads = n_threads < 1 ? 1 : (n_threads > 8 ? 8 : n_threads);
  std::vector<SequenceTable> tables(n_threads);
  std::vector<std::vector<uint64_t>> calls(n_threads, std::vector<uint64_t>(n_launchers, 0));
  std::atomic<size_t> next{0};
  std::vector<std::thread> workers;
  for (unsigned w = 0; w < n_threads; ++w)
    workers.emplace_back([&, w] {
      for (size_t i; (i = next.fetch_add(1)) < groups.size();) run_group(groups[i], tables[w], calls[w], nullptr);
    });
  for (std::thread& w : workers) w.join();
  if (launcher_names().size() != n_launchers) {
    fprintf(stderr, "a stub launcher is missing from register_launchers()\n");
    return 1;
  }
  SequenceTable all;
  std::vector<uint64_t> total(n_launchers, 0);
  for (unsigned w = 0; w < n_threads; ++w) {
    for (const auto& [h, sc] : tables[w]) {
      SequenceCount& dst = all[h];
      if (dst.count == 0) dst = SequenceCount{sc.launchers, sc.ret, 0};
      dst.count += sc.count;
    }
    for (size_t i = 0; i < n_launchers; ++i) total[i] += calls[w][i];
  }
  fprintf(out, "# launch routes of qlpc_dispatch.cpp over the grid of tests/host/dispatch_trace.cpp\n");
  fprintf(out, "# shapes:");
  for (int s = 0; s < kNumShapes; ++s) fprintf(out, " %d=%s", s, kShapes[s].name);
  fprintf(out, "\n# g <shape> <block size> <order> <cases> <hash of the full traces> <distinct launcher sequences>\n");
  for (const Group& g : groups)
    fprintf(out, "g %d %u %u %u %016" PRIx64 " %u\n", g.shape, g.block, g.order, g.cases, g.hash, g.sequences);
  fprintf(out, "# s <cases> <return> <launchers in call order>\n");
  std::vector<std::string> lines;
  for (const auto& [h, sc] : all) {
    std::string line = "s " + std::to_string(sc.count) + " " + error_name(sc.ret);
    for (uint16_t id : sc.launchers) line += " " + launcher_names()[id];
    lines.push_back(line);
  }
  // (ordered by text past the count, so that the table does not depend on the hash)
  std::sort(lines.begin(), lines.end(), [](const std::string& x, const std::string& y) {
    return x.substr(x.find(' ', 2)) < y.substr(y.find(' ', 2));
  });
  for (const std::string& line : lines) fprintf(out, "%s\n", line.c_str());
  fprintf(out, "# l <launcher> <calls>\n");
  for (size_t i = 0; i < n_launchers; ++i) fprintf(out, "l %s %" PRIu64 "\n", launcher_names()[i].c_str(), total[i]);
  return 0;
}

int dump(const char* spec) {
  char name[64];
  unsigned block = 0, order = 0;
  if (sscanf(spec, "%63[^:]:%u:%u", name, &block, &order) != 3) {
    fprintf(stderr, "--dump SHAPE:BLOCK:ORDER\n");
    return 2;
  }
  for (int s = 0; s < kNumShapes; ++s) {
    if (strcmp(kShapes[s].name, name) != 0 && std::to_string(s) != name) continue;
    Group g{s, block, order};
    SequenceTable table;
    std::vector<uint64_t> calls(launcher_names().size(), 0);
    std::string text;
    run_group(g, table, calls, &text);
    fputs(text.c_str(), stdout);
    printf("g %d %u %u %u %016" PRIx64 " %u\n", g.shape, g.block, g.order, g.cases, g.hash, g.sequences);
    return 0;
  }
  fprintf(stderr, "no such shape: %s\n", name);
  return 2;
}

}  // namespace
}  // namespace flacenc_hip

int main(int argc, char** argv) {
  flacenc_hip::register_launchers();
  if (argc == 3 && strcmp(argv[1], "--dump") == 0) return flacenc_hip::dump(argv[2]);
  if (argc == 3 && strcmp(argv[1], "--record") == 0) {
    FILE* out = fopen(argv[2], "w");
    if (!out) {
      perror(argv[2]);
      return 2;
    }
    const int rc = flacenc_hip::digests(out);
    return fclose(out) != 0 ? 2 : rc;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: dispatch_trace [--record FILE | --dump SHAPE:BLOCK:ORDER]\n");
    return 2;
  }
  return flacenc_hip::digests(stdout);
}
