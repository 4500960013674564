// api_internal.h -- what the translation units of the C ABI (include/flacenc_hip.h) share: the handle, its device
// buffers, the error helpers and the functions one unit calls in another.  Not installed, not part of any boundary.
//
// The handle owns the per-handle state the reference keeps in thread-locals (`reusable!`,
// src/lib.rs:92-116): the window cache (WINDOW_CACHE, src/lpc.rs:219-231) and
// the scratch buffers, here as device memory.  No allocation happens on the
// device-pointer path once the window for a block size is cached.
//
//   api_handle.cpp       create / destroy / synchronize, verify_config, pinned memory, set_error, ensure
//   api_windows.cpp      the analysis windows and their cache
//   api_candidates.cpp   the candidate batches: argument checks, scratch, the order mode's launches, enqueue, enqueue_fixed
//   frame_plan.cpp       pure, host-only testable: the records' config fields, the scratch rule, plan_frame_call
//   order_mode_core.h    pure: the order mode's step
//   api_frames.cpp       encode_frame's decisions: check, plan_frame_call, run the plan; wasted bits, encode + pack
//   api_pack.cpp         Frame::write, frame lengths, the wire format, stream offsets
//   api_stream.cpp       the streaming host path (flacenc_hip_encode_pcm)
//   api_decode.cpp       decode / verify / index
//   api_decode_stream.cpp  rows to packed PCM (flacenc_hip_pack_le_bytes), the streaming way back (flacenc_hip_decode_pcm)
//   flac_decode_ranges.cpp   sample ranges of a batch of streams (flacenc_hip_decode_ranges) on the index of stream_index.h
//   flac_decode_streams.cpp  a batch of streams to packed PCM (flacenc_hip_decode_streams, _md5): its kernels and the call
//   flac_recover_streams.cpp  a batch of damaged streams decoded through their errors (flacenc_hip_recover_streams)
//   md5_streams.cpp      MD5 digests of a batch of spans (flacenc_hip_md5_spans): its kernel, launcher and the call
//   encode_streams.cpp   a batch of PCM streams to frames (flacenc_hip_encode_streams): its kernels and the call
//   wide_encode.cpp      rows of up to 32 bits to frames (flacenc_hip_encode_pack_frames_wide): its kernels and the call
//   api_variable.cpp     the block-size search
//   api_debug_hooks.cpp  flacenc_hip_debug.h; linked into libflacenc_hip_hooks.so only
#ifndef FLACENC_HIP_API_INTERNAL_H_
#define FLACENC_HIP_API_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "comm.h"
#include "flacenc_hip.h"
#include "frame_pack.h"
#include "frame_plan.h"
#include "order_mode_core.h"
#include "qlpc_kernel.h"
#include "wide_encode_core.h"

namespace streamenc {
struct LaunchFrame;  // stream_encode_core.h
}

namespace flacenc_hip {

struct WindowEntry {
  uint32_t n;
  uint32_t type;
  uint32_t alpha_bits;
  uint32_t start, end;  // FLACENC_HIP_WINDOW_PARTIAL_TUKEY / _PUNCHOUT_TUKEY: the piece, in FLACENC_HIP_WINDOW_UNIT; else 0
  float* dev;  // 32 pad + rows*16 floats
  float* dev_lanes;  // n == 4096: the lane-major copy (window_lanes_core.h), behind `dev` in the same allocation; else nullptr
  int32_t flat_lo, flat_hi;
};

// an extra analysis window of FLACENC_HIP_FLAG_WINDOW_SEARCH (flacenc_hip_set_lpc_windows)
struct LpcWindow {
  uint32_t type;
  float alpha;
  uint32_t start, end;
};

// the default extra windows of a fresh handle (include/flacenc_hip.h, _capi.DEFAULT_LPC_WINDOWS)
const LpcWindow kDefaultLpcWindows[] = {
    {FLACENC_HIP_WINDOW_PARTIAL_TUKEY, 0.2f, 0, 36044},
    {FLACENC_HIP_WINDOW_PARTIAL_TUKEY, 0.2f, 29492, 65536},
    {FLACENC_HIP_WINDOW_PUNCHOUT_TUKEY, 0.2f, 0, 21845},
    {FLACENC_HIP_WINDOW_PUNCHOUT_TUKEY, 0.2f, 21845, 43690},
    {FLACENC_HIP_WINDOW_PUNCHOUT_TUKEY, 0.2f, 43690, 65536},
};

struct DeviceBuffer {
  void* ptr = nullptr;
  size_t cap = 0;
};

// Staging copies between ordinary (pageable) caller memory and the pinned slots of the streaming path: one
// memcpy stream moves ~20 GB/s on the host, well under what PCIe takes in both directions at once, so a
// copy is cut into slices for a few helper threads (the caller's thread takes one slice itself).
class CopyPool {
 public:
  explicit CopyPool(unsigned workers) : tasks_(workers) {
    try {
      threads_.reserve(workers);
      for (unsigned i = 0; i < workers; ++i) threads_.emplace_back([this, i] { run(i); });
    } catch (...) {  // a thread that did start must be joined before its std::thread is destroyed
      {
        std::lock_guard<std::mutex> g(m_);
        stop_ = true;
      }
      cv_.notify_all();
      for (std::thread& t : threads_) t.join();
      throw;
    }
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (std::thread& t : threads_) t.join();
  }
  unsigned workers() const { return static_cast<unsigned>(threads_.size()); }
  void copy(void* dst, const void* src, size_t n) {
    const size_t parts = threads_.size() + 1;
    if (threads_.empty() || n < (size_t(1) << 20)) {
      std::memcpy(dst, src, n);
      return;
    }
    const size_t slice = ((n + parts - 1) / parts + 4095) & ~size_t(4095);
    char* d = static_cast<char*>(dst);
    const char* sp = static_cast<const char*>(src);
    {
      std::lock_guard<std::mutex> g(m_);
      for (size_t i = 0; i < threads_.size(); ++i) {
        const size_t lo = (i + 1) * slice;
        const size_t len = lo >= n ? 0 : (n - lo < slice ? n - lo : slice);
        tasks_[i] = Task{d + lo, sp + lo, len};
      }
      pending_ = static_cast<unsigned>(threads_.size());
      ++generation_;
    }
    cv_.notify_all();
    std::memcpy(d, sp, slice < n ? slice : n);
    std::unique_lock<std::mutex> g(m_);
    done_cv_.wait(g, [this] { return pending_ == 0; });
  }

 private:
  struct Task {
    char* d = nullptr;
    const char* s = nullptr;
    size_t n = 0;
  };
  void run(unsigned idx) {
    unsigned long long seen = 0;
    for (;;) {
      Task t;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return stop_ || generation_ != seen; });
        if (stop_) return;
        seen = generation_;
        t = tasks_[idx];
      }
      if (t.n) std::memcpy(t.d, t.s, t.n);
      {
        std::lock_guard<std::mutex> g(m_);
        --pending_;
      }
      done_cv_.notify_one();
    }
  }
  std::vector<std::thread> threads_;
  std::vector<Task> tasks_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  unsigned long long generation_ = 0;
  unsigned pending_ = 0;
  bool stop_ = false;
};

}  // namespace flacenc_hip

struct flacenc_hip_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  std::vector<flacenc_hip::WindowEntry> windows;
  // FLACENC_HIP_FLAG_WINDOW_SEARCH: the extra analysis windows (windows 1 .. W-1; window 0 is the config's)
  std::vector<flacenc_hip::LpcWindow> lpc_windows{std::begin(flacenc_hip::kDefaultLpcWindows), std::end(flacenc_hip::kDefaultLpcWindows)};
  flacenc_hip::DeviceBuffer d_samples, d_residual, d_params, d_bps, d_autocorr, d_lpc, d_tables, d_keys, d_sel, d_results, d_out, d_outlen, d_cparams, d_cresid, d_fparams, d_fresid, d_fkeys, d_split, d_presid, d_sumabs, d_minmax, d_marked, d_irlsw, d_gram;
  flacenc_hip::DeviceBuffer d_dec, d_dec_io, d_idx;  // frame decoder: skim records, host-pointer staging, index candidates
  // pack_le_bytes: the offsets when the caller wants none, host-pointer staging; decode_pcm: a window's index
  flacenc_hip::DeviceBuffer d_ppk_off, d_ppk_io, d_dpcm_idx;
  flacenc_hip::DeviceBuffer d_md5;  // md5_spans: the span table and (host pointers) the digests
  flacenc_hip::DeviceBuffer d_encs;  // encode_streams: the plan's tables, lengths, offsets and totals
  // block-size search: the levels' frames, decision records and packed frames, its own records, host-pointer staging
  flacenc_hip::DeviceBuffer d_vbs_frames, d_vbs_results, d_vbs_pack, d_vbs_meta, d_vbs_io;
  // wasted bits: k per row, the marked frames (count first), the shifted rows and their widths
  flacenc_hip::DeviceBuffer d_wk, d_wlist, d_wrows, d_wbps;
  // order / window search: every window's R[], every candidate's predictor record and the choice (order_search.h)
  flacenc_hip::DeviceBuffer d_order;
  flacenc_hip::DeviceBuffer d_wide;  // the wide encode path's records, one per (frame, role) (wide_encode.cpp)
  flacenc_hip::DeviceBuffer d_esc;  // the packers' list of frames with escaped partitions (FramePackArgs::escape_list)
  uint32_t order_guesses = 1;  // FLACENC_HIP_FLAG_ORDER_GUESS: K, the guesses per window (flacenc_hip_set_order_guesses)
  // FLACENC_HIP_FLAG_PRECISION_SEARCH: F, the lowest precision searched (flacenc_hip_set_precision_floor)
  uint32_t precision_floor = 5;
  // the deepest stream the decode calls take, 24 or 32 (flacenc_hip_set_max_bits_per_sample)
  uint32_t max_bps = 24;
  // the deepest PCM the stream-level encode calls take, 24 or 32 (flacenc_hip_set_max_encode_bits_per_sample)
  uint32_t max_encode_bps = 24;
  // streaming host path (flacenc_hip_encode_pcm_stereo): copy-in / copy-out streams, two slots of pinned
  // staging and device buffers, the events that order them
  uint32_t marked_parity = 0;  // which of d_marked's two counters the current pipeline counts into
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_fill[2] = {nullptr, nullptr}, ev_pack[2] = {nullptr, nullptr},
             ev_d2h[2] = {nullptr, nullptr};
  flacenc_hip::DeviceBuffer d_pcm[2], d_pack[2], d_plen[2], d_poff[2], d_cont[2];
  void* pin_in[2] = {nullptr, nullptr};
  void* pin_out[2] = {nullptr, nullptr};
  void* pin_meta[2] = {nullptr, nullptr};
  size_t pin_in_cap = 0, pin_out_cap = 0, pin_meta_cap = 0;
  int host_threads = -1;  // staging-copy threads of the streaming path: -1 = default, see flacenc_hip_set_host_threads
  std::unique_ptr<flacenc_hip::CopyPool> copy_pool;
  unsigned long long* stamps = nullptr;  // profiling hook, see flacenc_hip_debug_set_stamps
  unsigned long long* fixed_keys = nullptr;  // test hook, see flacenc_hip_debug_set_fixed_keys
  uint32_t* cert_stats = nullptr;  // statistics hook, see flacenc_hip_debug_set_cert_stats
  void* order_guess_trace = nullptr;  // test hook, see flacenc_hip_debug_set_order_guess_trace
  // test hook, see flacenc_hip_debug_set_stream_chunk: frames per chunk of the streaming path in place of its rule (0:
  // the rule; nothing in the product library sets it), and the plan of the last flacenc_hip_encode_pcm* call
  size_t stream_chunk_override = 0;
  size_t last_stream_chunk = 0, last_stream_chunks = 0;
  bool last_stream_in_pinned = false, last_stream_out_pinned = false;  // how that call took the caller's buffers
  // test hook, see flacenc_hip_debug_set_decode_plan: window bytes and frames per group of flacenc_hip_decode_pcm in
  // place of its rules (0: the rule), and the plan the last call ran
  size_t decode_window_override = 0, decode_group_override = 0;
  size_t last_decode_window = 0, last_decode_windows = 0, last_decode_group = 0, last_decode_groups = 0;
  // test hook, see flacenc_hip_debug_last_decode_streams_plan: kernel launches, host synchronisations, host-device
  // transfers and channel classes of the last flacenc_hip_decode_streams / flacenc_hip_decode_streams_md5 call
  uint64_t last_streams_plan[4] = {0, 0, 0, 0};
  // flacenc_hip_decode_ranges: the range table in rslot order on its way to the device, and (test hook, see
  // flacenc_hip_debug_last_decode_ranges_plan) launches, synchronisations, transfers and the ranges' channel classes
  std::vector<char> ranges_table;
  uint64_t last_ranges_plan[4] = {0, 0, 0, 0};
  // test hook, see flacenc_hip_debug_last_recover_plan: the same four words of the last flacenc_hip_recover_streams call
  uint64_t last_recover_plan[4] = {0, 0, 0, 0};
  // test hooks, see flacenc_hip_debug_set_encode_streams_chunk / flacenc_hip_debug_last_encode_streams_plan: frames per
  // frame-level call of flacenc_hip_encode_streams in place of its rule (0: the rule), and what the last call did
  size_t encode_streams_chunk_override = 0;
  uint64_t last_encode_streams_plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // test hook, see flacenc_hip_debug_last_search_slices: the slices of the last order / window / precision search launch
  uint32_t last_search_slices = 0;
  // measurement hook, see flacenc_hip_debug_set_planar_fill_form: how planar_fill_kernel loads (1 aligned 16-byte loads
  // brought into place, the product's form: the faster one; 0 dwords)
  int planar_fill_form = 1;
  flacenc_hip::CommState* comm = nullptr;  // RCCL communicator of the ordered gather (comm.cpp)
  // Order mode of the certified shapes by material (launch_adaptive, order_mode_core.h): the certificate's own counters
  // of the last launches, cumulative on the device and mirrored into one pinned word by a one-thread kernel behind each
  struct OrderMode {
    uint32_t* d_counters = nullptr;         // device: the three counters of QlpcKernelArgs::cert_stats
    unsigned long long* verdict = nullptr;  // pinned, device-visible: the latest verdict (cert_feedback_kernel)
    order_mode::State state;
    int enabled = 1;                        // flacenc_hip_debug_set_adaptive_order(h, 0) pins the certified kernel
  } adaptive;
};

#define HIP_TRY(h, expr)                          \
  do {                                            \
    hipError_t err__ = (expr);                    \
    if (err__ != hipSuccess) {                    \
      flacenc_hip::set_error((h), #expr, err__);  \
      return FLACENC_HIP_ERR_DEVICE;              \
    }                                             \
  } while (0)

namespace planarenc {
struct Frame;
struct Stream;
}  // namespace planarenc

namespace flacenc_hip {

// ---- api_handle.cpp ----
bool set_error(flacenc_hip_handle* h, const char* what, hipError_t err);
// grows by 25 % + 256 bytes, frees what it held: the contents do not survive
int ensure(flacenc_hip_handle* h, DeviceBuffer& b, size_t bytes);
// every DeviceBuffer the handle owns: what flacenc_hip_destroy frees and flacenc_hip_debug_scratch_bytes reports
std::vector<DeviceBuffer*> device_buffers(flacenc_hip_handle* h);
// the tail of a blocking call on device pointers: the async entry's code, or the handle's stream drained
int drained(flacenc_hip_handle* h, int rc, bool nothing_queued);
// the blocking calls on host pointers: `n_rows` rows of `block_size` words between the caller's buffer (row stride
// `stride` words) and handle scratch at padded_stride(block_size), on the handle's stream
int rows_to_device(flacenc_hip_handle* h, const DeviceBuffer& b, const int32_t* rows, size_t stride, uint32_t block_size,
                   size_t n_rows);
int rows_to_host(flacenc_hip_handle* h, int32_t* rows, size_t stride, const DeviceBuffer& b, uint32_t block_size,
                 size_t n_rows);

// (padded_stride, frame_plan.h: the row stride of every scratch buffer of sample or residual rows, whole 16-byte groups)
inline size_t a256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// ---- api_windows.cpp ----
int get_window_entry(flacenc_hip_handle* h, uint32_t type, float alpha, uint32_t start, uint32_t end, uint32_t n,
                     const WindowEntry** out);
int get_window(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, uint32_t n, const WindowEntry** out);

// ---- api_candidates.cpp ----
int check_batch_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, const int32_t* samples,
                     size_t n_subframes, uint32_t block_size, size_t stride, flacenc_hip_subframe_params* params,
                     int32_t* residual, size_t residual_stride, uint32_t min_block = FLACENC_HIP_MIN_BLOCK_SIZE);
int check_bits_per_sample(flacenc_hip_handle* h, uint32_t bits_per_sample);  // 8..=24
int verify_fixed(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg);
// config_record (frame_plan.h) + what the handle adds: the window entry (`win` null: no window, flat range 0) and the
// statistics hook.  Everything else is as QlpcKernelArgs initialises it; each caller sets what is its own.
QlpcKernelArgs base_args(flacenc_hip_handle* h, const flacenc_hip_qlpc_config& q, const WindowEntry* win,
                         const int32_t* samples, size_t stride, uint32_t block_size, size_t n_subframes,
                         const uint8_t* bps, uint32_t bps_uniform, bool stereo);
// gives the record what scratch_grant (frame_plan.h) says
int attach_scratch(flacenc_hip_handle* h, QlpcKernelArgs& a, ScratchGrant grant, hipStream_t stream);
int launch_adaptive(flacenc_hip_handle* h, const QlpcKernelArgs& a, const QlpcLaunchPlan& plan, hipStream_t stream);
// The candidates' scratch of a frame-level call in the handle's buffers, named as the deciding kernels' records name it:
// records, rows at padded_stride(block_size), on request the roles' min / max, the selector keys; null where a kind is off
struct Candidates {
  flacenc_hip_subframe_params *lpc_params = nullptr, *fixed_params = nullptr;
  int32_t *lpc_residual = nullptr, *fixed_residual = nullptr, *minmax = nullptr;
  unsigned long long* fixed_keys = nullptr;
  bool placed = false;  // CandidateBatch::placed of the LPC batch
};
int candidate_scratch(flacenc_hip_handle* h, size_t n_rows, uint32_t block_size, bool lpc, bool fixed, bool with_minmax,
                      Candidates* out);
// One candidate batch, estimated_qlpc (enqueue) resp. fixed_lpc (enqueue_fixed): a call site gives the rows and names the rest
struct CandidateBatch {
  CandidateBatch(const int32_t* rows, size_t n, uint32_t block, size_t row_stride, const uint8_t* widths = nullptr)
      : samples(rows), n_subframes(n), stride(row_stride), block_size(block), bps(widths) {}
  void write_to(flacenc_hip_subframe_params* records, int32_t* rows, size_t row_stride) {
    params = records;
    residual = rows;
    residual_stride = row_stride;
  }
  const int32_t* samples;  // the rows: n_subframes of block_size words, `stride` words apart
  size_t n_subframes, stride;
  uint32_t block_size;
  const uint8_t* bps;            // per-row widths, or (null) bps_uniform for all
  uint32_t bps_uniform = 16;
  bool stereo = false;           // rows 4f .. 4f + 3 are the roles of 2-channel frame f
  flacenc_hip_subframe_params* params = nullptr;  // out: the records, the rows
  int32_t* residual = nullptr;
  size_t residual_stride = 0;
  double *autocorr = nullptr, *lpc_coefs = nullptr;  // optional outputs of enqueue ...
  unsigned long long* selector_keys = nullptr;       // ... and of enqueue_fixed
  // frame-level callers on the big-block shapes (QlpcKernelArgs::residual_lr, ::residual_mode): L / R candidates straight
  // into the frame's rows with the roles' min / max, or (analyse_only) records and min / max alone
  int32_t *residual_lr = nullptr, *minmax_out = nullptr;
  size_t residual_lr_stride = 0;
  bool analyse_only = false;
  bool placed = false;  // out: enqueue did so (the big-block kernels took the launch)
};
int enqueue(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, CandidateBatch& b, hipStream_t stream);
int enqueue_fixed(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, CandidateBatch& b, hipStream_t stream);

// ---- api_stream.cpp ----
// what the streaming host paths (encode_pcm, decode_pcm) share: is the caller's buffer page-locked, the two pinned
// slots of a staging buffer, the copy streams and events, the helper threads of the staging copies
bool is_pinned(const void* p);
int ensure_pinned(flacenc_hip_handle* h, void** slot, size_t* cap_field, size_t bytes);
int ensure_stream_objects(flacenc_hip_handle* h);
int ensure_copy_pool(flacenc_hip_handle* h, const char* what);

// ---- md5_streams.cpp ----
// One lane per span: the MD5 of bytes[offsets[i * offset_stride] .. + lengths[i]) to digests + 16 * slot[i] (lengths null:
// every span empty; slot null: digests + 16 * i).  All pointers are device memory; one launch on `stream`, none for
// n_spans == 0.
hipError_t launch_md5_spans(const uint8_t* bytes, const uint64_t* offsets, uint32_t offset_stride,
                            const uint64_t* lengths, const uint32_t* slot, uint32_t n_spans, uint8_t* digests,
                            hipStream_t stream);

// ---- encode_streams.cpp ----
// streams_fill_kernel on `stream`: frames table[0 .. n_frames) into rows row0 .. of `rows` (channel-major, `stride` words
// per row, stride a multiple of 4, rows 16-byte aligned).  All pointers are device memory; one launch.
hipError_t launch_streams_fill(const uint8_t* pcm, const streamenc::LaunchFrame* table, uint32_t n_frames,
                               uint32_t channels, uint32_t bytes_per_sample, uint32_t row0, size_t stride, int32_t* rows,
                               hipStream_t stream);

// Both flacenc_hip_encode_streams (planar null) and flacenc_hip_encode_streams_planar (pcm null): the one body.
struct PlanarSource {
  const void* samples;
  uint64_t samples_bytes;
  uint32_t sample_format;
  uint64_t row_pitch;
  uint8_t* digests;   // null: no packed image is built
  uint64_t* clipped;  // null: not counted
};
int encode_streams_common(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm, uint64_t pcm_bytes,
                          const PlanarSource* planar, const void* streams, size_t n_streams, uint32_t block_size,
                          uint8_t* out, uint64_t out_bytes, uint32_t* frame_lengths, size_t max_frames, uint64_t* totals,
                          uint64_t call_totals[2], int memory_kind);

// ---- encode_streams_planar.cpp ----
// planar_fill_kernel on `stream`: what launch_streams_fill does, from rows of 4-byte elements (`elems` + Frame::elem0 +
// c * Frame::pitch) of format `sample_format`, float32 quantised to `bits` bits; clipped (null: not counted) gets the
// elements per stream that clamped or were NaN.  One launch.
hipError_t launch_planar_fill(const uint32_t* elems, const planarenc::Frame* table, uint32_t n_frames, uint32_t channels,
                              uint32_t sample_format, uint32_t bits, uint32_t row0, size_t stride, int32_t* rows,
                              unsigned long long* clipped, int form, hipStream_t stream);
// planar_pack_kernel: the packed interleaved little-endian PCM of every stream of the table, at Stream::packed_base of
// `image`; `per` is the most dwords a frame starts.  One launch for all classes.
hipError_t launch_planar_pack(const uint32_t* elems, const planarenc::Frame* table, uint32_t n_frames,
                              const planarenc::Stream* streams, const flacenc_hip_pcm_stream_desc* descs, uint32_t per,
                              uint32_t sample_format, uint8_t* image, hipStream_t stream);

// ---- flac_recover_streams.cpp ----
// The segmented inclusive max-scan of flacenc_hip_recover_streams on `stream`: segmax_reduce_kernel, segmax_carry_kernel
// and segmax_apply_kernel, sized by max_frames, over the counters[C_FRAMES] <= max_frames elements of a frame sequence.
// Element m is a head where m == base[f_slot[m]]; emax[m] goes in as its value and comes out as the maximum from its
// segment's head up to m.  agg_h, agg_v: ceil(max_frames / 256) words of scratch.  All pointers are device memory;
// three launches, counted in plan[0].
hipError_t launch_segmax_scan(uint64_t* plan, const uint32_t* f_slot, const uint64_t* base, uint64_t* emax,
                              const uint32_t* counters, size_t max_frames, uint32_t* agg_h, uint64_t* agg_v,
                              hipStream_t stream);

// ---- wide_encode.cpp ----
// The wide encode path's launch record: rows in, frame bytes and lengths out (wide_encode_core.h holds the rule).
struct WideEncodeArgs {
  const int32_t* frames;  // n_frames * channels rows of block_size words, `stride` words apart
  size_t stride;
  uint32_t channels, block_size, bits_per_sample, sample_rate;
  uint32_t n_frames, first_frame_number, frame_number_step;
  wideenc::Config cfg;
  wideenc::SubRecord* records;  // scratch: n_frames * roles_of(channels)
  uint8_t* out;                 // 16-byte aligned slots of out_stride bytes
  size_t out_stride;
  uint32_t* out_len;
};
// wide_decide_kernel and wide_write_kernel on `stream`; all pointers are device memory.
hipError_t launch_wide_encode(const WideEncodeArgs& a, hipStream_t stream);
// the device step enqueued on `stream` (flacenc_hip_encode_pack_frames_wide is its blocking form on the handle's stream)
int encode_pack_frames_wide(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                            size_t n_frames, uint32_t channels, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                            uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                            size_t out_stride, uint32_t* out_len, hipStream_t stream);
// does a class of `bits_per_sample` run the wide step in the stream-level calls
inline bool is_wide(uint32_t bits_per_sample) { return bits_per_sample > 24; }

// ---- api_pack.cpp ----
void fill_crc_powers(uint32_t lds_words, uint32_t* crc_per, uint16_t crc_pow[32]);
void fill_header_specs(FramePackArgs& a, uint32_t block_size, uint32_t sample_rate, uint32_t bits_per_sample);

}  // namespace flacenc_hip
#endif
