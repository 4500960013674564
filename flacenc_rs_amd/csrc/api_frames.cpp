// api_frames.cpp -- encode_frame's decisions for batches of frames: Independent(channels) frames, 2-channel frames with
// the stereo decision, FLACENC_HIP_FLAG_WASTED_BITS around both, and the encode + pack calls.
#include "api_internal.h"
#include "frame_decide.h"
#include "wasted_bits.h"

using namespace flacenc_hip;

namespace {

struct PackTarget {  // optional: where the fused kernel puts the packed frames
  uint8_t* out = nullptr;
  size_t out_stride = 0;
  uint32_t* out_len = nullptr;
  uint32_t sample_rate = 0, first_frame_number = 0, frame_number_step = 1;
};
int encode_stereo_frames_impl(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                              size_t n_frames, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                              flacenc_hip_stereo_frame_result* results, int32_t* residual, size_t residual_stride,
                              void* stream, const PackTarget* pack, bool* packed);

// The config a frame-level call runs with: the window search without windows and the precision search without a
// precision below quant_precision normalised away (search_flags), and
// too_short (coding.rs:396): neither fixed_lpc nor estimated_qlpc is tried; Constant or Verbatim
flacenc_hip_frame_config frame_config(const flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, uint32_t block_size) {
  flacenc_hip_frame_config c = *cfg;
  c.qlpc.flags = search_flags(h, cfg->qlpc.flags, cfg->qlpc.quant_precision);
  if (block_size < FLACENC_HIP_MIN_BLOCK_SIZE) c.use_fixed = c.use_lpc = 0;
  return c;
}

// QlpcKernelArgs::fixed_group_log2 of the fused kernels: with the ApproxEnt selector the estimator's partitions must be
// whole groups of 64-sample lanes, 2^g lanes each.  *composite: they are not (a partition count that is no power of
// two) and the launch takes the general path.  (`cfg` has passed verify_fixed: 1..=64 partitions.)
uint32_t fixed_group_log2(const flacenc_hip_frame_config* cfg, bool* composite) {
  *composite = false;
  if (!cfg->use_fixed || cfg->fixed_order_sel != FLACENC_HIP_ORDERSEL_APPROXENT) return 0;
  const uint32_t p = cfg->fixed_partitions;
  *composite = (p & (p - 1)) != 0;
  uint32_t g = 0;
  for (uint32_t lanes = *composite ? 1u : 64u / p; lanes > 1; lanes >>= 1) ++g;
  return g;
}

// The launch record of a frame-level call over `n_sub` rows of one width: base_args with the config's window (none
// for a short block, which never reads it: short blocks take the candidate-free general path), the output rows and
// encode_frame's switches.  The caller names its results (frame_results / chan_results) and, stereo, the stamps.
int frame_args(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames, size_t n_sub,
               uint32_t block_size, size_t stride, uint32_t bits_per_sample, bool stereo, int32_t* residual,
               size_t residual_stride, uint32_t group_log2, QlpcKernelArgs* out) {
  const WindowEntry* win = nullptr;
  if (block_size >= FLACENC_HIP_MIN_BLOCK_SIZE) {
    int rc = get_window(h, &cfg->qlpc, block_size, &win);
    if (rc != FLACENC_HIP_OK) return rc;
  }
  QlpcKernelArgs a = base_args(h, cfg->qlpc, win, frames, stride, block_size, n_sub, nullptr, bits_per_sample, stereo);
  a.residual = residual;
  a.residual_stride = residual_stride;
  a.use_constant = cfg->use_constant;
  a.use_lpc = cfg->use_lpc;
  a.use_leftside = stereo ? cfg->use_leftside : 0;
  a.use_rightside = stereo ? cfg->use_rightside : 0;
  a.use_midside = stereo ? cfg->use_midside : 0;
  a.use_fixed = cfg->use_fixed;
  a.fixed_max_order = cfg->fixed_max_order;
  a.fixed_order_sel = cfg->fixed_order_sel;
  a.fixed_group_log2 = group_log2;
  a.fixed_keys = h->fixed_keys;
  *out = a;
  return FLACENC_HIP_OK;
}

// qlpc_subwave_kernel's frame variants on blocks of 8 / 16 / 32 finest Rice partitions (512 .. 2304 samples), and the
// clean-up of what they marked.  The kernel does the whole of encode_frame (`fd`: 2-channel frames, both candidates of
// the four roles, the decision, the two chosen rows) resp. encode_subframe of every channel (`cd`: independent
// channels) in one launch, several frames per workgroup.  A frame (a subframe) with a candidate beyond its exact sums
// (residuals of 2^25 and more) comes back marked and takes the general path, restricted to what is marked: the QLPC
// clean-up, the fixed_lpc clean-up and the deciding kernel, three launches that return at once when the count is 0.
// Exactly one of `fd` / `cd` is given, filled but for the candidates.  *taken = false: not this kernel's launch (the
// split scratch has been attached all the same).
int subwave_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const QlpcKernelArgs& a,
                   FrameDecideArgs* fd, ChannelDecideArgs* cd, hipStream_t s, bool* taken) {
  *taken = false;
  int rc;
  QlpcKernelArgs m = a;
  m.stamps = nullptr;
  m.fixed_partitions = cfg->fixed_partitions;
  // (the unflagged order on these shapes is the reference's: its chains for every QLPC candidate in front, QlpcKernelArgs::cert_subwave)
  m.cert_subwave = (a.certify != 0u && a.reference_order == 0u && !a.direct_mse && cfg->use_lpc && cfg->qlpc.lpc_order <= 12) ? 1u : 0u;
  if ((rc = attach_split_scratch(h, m, s)) != FLACENC_HIP_OK) return rc;
  m.marked_unit = fd ? 4 : 1;  // (the frame variant lists marked FRAMES; the candidate clean-ups visit their four roles)
  if (!(fd ? subwave_frame_eligible(m) : subwave_channels_eligible(m))) return FLACENC_HIP_OK;
  *taken = true;
  LpcScratch lpc;
  FixedScratch fixed{};
  if ((rc = lpc_scratch(h, a.n_subframes, a.block_size, false, &lpc)) != FLACENC_HIP_OK) return rc;
  m.cand_lpc_params = lpc.params;
  if (cfg->use_fixed) {
    if ((rc = fixed_scratch(h, a.n_subframes, a.block_size, &fixed)) != FLACENC_HIP_OK) return rc;
    m.cand_fixed_params = fixed.params;
  }
  HIP_TRY(h, launch_subwave_frames(m, s));
  // the marked candidates, by the generic kernel's clean-up launches (status -1 in the scratch records)
  QlpcKernelArgs c = m;
  c.frame_results = nullptr;
  c.chan_results = nullptr;
  c.cand_lpc_params = c.cand_fixed_params = nullptr;
  c.params = lpc.params;
  c.residual = lpc.rows;
  c.residual_stride = padded_stride(a.block_size);
  c.only_marked = 1;
  c.use_fixed = 0;
  c.fixed_keys = nullptr;
  HIP_TRY(h, launch_qlpc(c, plan_qlpc_launch(a.block_size, cfg->qlpc.lpc_order), s));
  if (cfg->use_fixed) {
    QlpcKernelArgs x = c;
    x.params = fixed.params;
    x.residual = fixed.rows;
    x.selector_keys = fixed.keys;
    x.window = nullptr;
    x.window_lanes = nullptr;
    x.flat_lo = x.flat_hi = 0;
    x.lpc_order = 4;
    x.precision = 0;
    x.use_fixed = 1;
    x.fixed_mode = 1;
    HIP_TRY(h, launch_qlpc(x, plan_qlpc_launch(a.block_size, 4), s));
  }
  // (the two deciding kernels' records name the candidates and the marked list alike; entries: frames resp. subframes)
  auto marked_candidates = [&](auto& d) {
    d.lpc_params = lpc.params;
    d.lpc_residual = lpc.rows;
    d.fixed_params = fixed.params;
    d.fixed_residual = fixed.rows;
    d.fixed_keys = fixed.keys;
    d.only_marked = 1;
    d.marked_count = m.marked_count;
    d.marked_list = m.marked_list;
    d.marked_cap = m.marked_cap;
  };
  if (fd) {
    marked_candidates(*fd);
    HIP_TRY(h, launch_frame_decide(*fd, s));
  } else {
    marked_candidates(*cd);
    HIP_TRY(h, launch_channel_decide(*cd, s));
  }
  return FLACENC_HIP_OK;
}

// FLACENC_HIP_FLAG_WASTED_BITS for stereo frames (channels == 0) or Independent(channels) frames: scan, one host
// synchronisation for the count m of frames with wasted bits, the unflagged pipeline unless every frame has some, then
// the fix-up of the m frames -- their rows x >> k through the candidate batches (per-row width w - k) and a deciding
// kernel that writes their records and residual rows over the first pass's.  Device pointers, `stream`.
int encode_wasted(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames, size_t n_frames,
                  uint32_t channels, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                  flacenc_hip_stereo_frame_result* results, flacenc_hip_channel_result* chan_results, int32_t* residual,
                  size_t residual_stride, void* stream) {
  const bool stereo = channels == 0;
  const size_t rows = stereo ? 4 : channels;
  int rc = check_batch_args(h, &cfg->qlpc, frames, n_frames * rows, block_size, stride,
                            stereo ? reinterpret_cast<flacenc_hip_subframe_params*>(results)
                                   : reinterpret_cast<flacenc_hip_subframe_params*>(chan_results),
                            residual, residual_stride, 1);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  if (bits_per_sample < 8 || bits_per_sample > 24) {
    h->last_error = "bits_per_sample must be in 8..=24";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (cfg->use_fixed && (rc = verify_fixed(h, cfg)) != FLACENC_HIP_OK) return rc;
  // the unflagged configuration (FUSED_PACK: a kernel choice the fix-up's packer has no part in)
  flacenc_hip_frame_config plain = *cfg;
  plain.qlpc.flags = search_flags(h, plain.qlpc.flags, plain.qlpc.quant_precision) & ~(FLACENC_HIP_FLAG_WASTED_BITS | FLACENC_HIP_FLAG_FUSED_PACK);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = ensure(h, h->d_wk, n_frames * rows)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_wlist, (n_frames + 1) * 4)) != FLACENC_HIP_OK) return rc;
  WastedArgs w{};
  w.frames = frames;
  w.stride = stride;
  w.block_size = block_size;
  w.n_frames = static_cast<uint32_t>(n_frames);
  w.channels = stereo ? 2u : channels;
  w.stereo = stereo ? 1u : 0u;
  w.bits_per_sample = bits_per_sample;
  w.k = static_cast<uint8_t*>(h->d_wk.ptr);
  w.count = static_cast<uint32_t*>(h->d_wlist.ptr);
  w.list = w.count + 1;
  w.use_constant = cfg->use_constant;
  HIP_TRY(h, hipMemsetAsync(w.count, 0, 4, s));
  HIP_TRY(h, launch_wasted_scan(w, s));
  uint32_t m = 0;
  HIP_TRY(h, hipMemcpyAsync(&m, w.count, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (m < n_frames) {  // (m = 0: exactly the unflagged launches)
    rc = stereo ? encode_stereo_frames_impl(h, &plain, frames, n_frames, block_size, stride, bits_per_sample, results,
                                            residual, residual_stride, stream, nullptr, nullptr)
                : flacenc_hip_encode_frames_async(h, &plain, frames, n_frames, channels, block_size, stride,
                                                  bits_per_sample, chan_results, residual, residual_stride, stream);
    if (rc != FLACENC_HIP_OK || m == 0) return rc;
  }
  // ---- the fix-up of the m marked frames ----
  if (block_size < FLACENC_HIP_MIN_BLOCK_SIZE) plain.use_fixed = plain.use_lpc = 0;  // too_short, coding.rs:396
  const size_t n_rows = static_cast<size_t>(m) * rows;
  const size_t cstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_wrows, n_rows * cstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_wbps, n_rows)) != FLACENC_HIP_OK) return rc;
  w.m = m;
  w.shifted = static_cast<int32_t*>(h->d_wrows.ptr);
  w.shifted_stride = cstride;
  w.shifted_bps = static_cast<uint8_t*>(h->d_wbps.ptr);
  w.use_fixed = plain.use_fixed;
  w.use_lpc = plain.use_lpc;
  w.use_leftside = plain.use_leftside;
  w.use_rightside = plain.use_rightside;
  w.use_midside = plain.use_midside;
  w.cand_stride = cstride;
  w.results = results;
  w.chan_results = chan_results;
  w.residual = residual;
  w.residual_stride = residual_stride;
  HIP_TRY(h, launch_wasted_shift(w, s));
  if (plain.use_lpc) {  // estimated_qlpc of the shifted rows: what flacenc_hip_qlpc_batch runs
    LpcScratch lpc;
    if ((rc = lpc_scratch(h, n_rows, block_size, false, &lpc)) != FLACENC_HIP_OK) return rc;
    rc = enqueue(h, &plain.qlpc, w.shifted, n_rows, block_size, cstride, w.shifted_bps, lpc.params, lpc.rows, cstride,
                 nullptr, nullptr, s);
    if (rc != FLACENC_HIP_OK) return rc;
    w.lpc_params = lpc.params;
    w.lpc_residual = lpc.rows;
  }
  if (plain.use_fixed) {  // fixed_lpc of the shifted rows: what flacenc_hip_fixed_lpc_batch runs
    FixedScratch fixed;
    if ((rc = fixed_scratch(h, n_rows, block_size, &fixed)) != FLACENC_HIP_OK) return rc;
    rc = enqueue_fixed(h, &plain, w.shifted, n_rows, block_size, cstride, w.shifted_bps, bits_per_sample, false,
                       fixed.params, fixed.rows, cstride, fixed.keys, s);
    if (rc != FLACENC_HIP_OK) return rc;
    w.fixed_params = fixed.params;
    w.fixed_residual = fixed.rows;
    w.fixed_keys = fixed.keys;
  }
  HIP_TRY(h, launch_wasted_decide(w, s));
  return FLACENC_HIP_OK;
}

// Frame::write inside the deciding wave kernel: the header constants and CRC powers of `pack` into the launch record.
// Leaves a.pack_out null when the frame's bit buffer does not fit where the kernel keeps it.
void attach_fused_pack(QlpcKernelArgs& a, const PackTarget* pack, uint32_t bits_per_sample) {
  const size_t bound = flacenc_hip_stereo_frame_bytes_bound(a.block_size, bits_per_sample);
  FramePackArgs pa{};
  fill_header_specs(pa, a.block_size, pack->sample_rate, bits_per_sample);
  a.pack_out = pack->out;
  a.pack_out_stride = pack->out_stride;
  a.pack_out_len = pack->out_len;
  a.pack_header_mid = pa.header_mid;
  a.pack_extra_len = pa.extra_len;
  for (int i = 0; i < 4; ++i) a.pack_extra[i] = pa.extra[i];
  a.pack_first_frame = pack->first_frame_number;
  a.pack_frame_step = pack->frame_number_step;
  a.pack_lds_words = static_cast<uint32_t>(bound / 4 + 4);
  fill_crc_powers(a.pack_lds_words, &a.pack_crc_per, a.pack_crc_pow);
  if (static_cast<size_t>(a.pack_lds_words) * 4 > 35424) a.pack_out = nullptr;  // the bit buffer reuses the two channel images
}

// Big-block shapes: two analyse-only passes (QLPC, fixed_lpc: records, no residual rows), then one kernel that
// decides and writes only the two rows the frame keeps (bigblock_residual_kernel, modes 1 and 2) -- eight candidate
// rows per frame stay off HBM, and so does the copy of the chosen two.
bool big_block_frames(const flacenc_hip_frame_config* cfg, const QlpcKernelArgs& a) {
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

int encode_big_block_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const QlpcKernelArgs& a,
                            hipStream_t s) {
  const size_t n_sub = a.n_subframes, cstride = padded_stride(a.block_size);
  int rc;
  LpcScratch lpc;
  if ((rc = lpc_scratch(h, n_sub, a.block_size, true, &lpc)) != FLACENC_HIP_OK) return rc;
  bool analysed = false;
  rc = enqueue(h, &cfg->qlpc, a.samples, n_sub, a.block_size, a.stride, nullptr, lpc.params, lpc.rows, cstride, nullptr,
               nullptr, s, true, a.bps_uniform, nullptr, 0, lpc.minmax, &analysed, 1u);
  if (rc != FLACENC_HIP_OK) return rc;
  if (!analysed) {
    h->last_error = "internal: analyse-only QLPC batch on a shape the big-block kernels do not take";
    return FLACENC_HIP_ERR_UNSUPPORTED;
  }
  QlpcKernelArgs m = a;  // (shape, width, the frame's results and rows and the encode_frame switches are set there)
  m.residual_mode = 2u;
  m.stamps = nullptr;
  m.cand_lpc_params = lpc.params;
  m.cand_lpc_rows = lpc.rows;
  m.cand_minmax = lpc.minmax;
  m.cand_stride = cstride;
  if (cfg->use_fixed) {
    FixedScratch fixed;
    if ((rc = fixed_scratch(h, n_sub, a.block_size, &fixed)) != FLACENC_HIP_OK) return rc;
    rc = enqueue_fixed(h, cfg, a.samples, n_sub, a.block_size, a.stride, nullptr, a.bps_uniform, true, fixed.params,
                       fixed.rows, cstride, fixed.keys, s, 1u);
    if (rc != FLACENC_HIP_OK) return rc;
    m.cand_fixed_params = fixed.params;
    m.cand_fixed_rows = fixed.rows;
    m.cand_fixed_keys = fixed.keys;
  }
  HIP_TRY(h, launch_bigblock_residual(m, s));
  return FLACENC_HIP_OK;
}

// General shapes: the same result from candidate batches (4 QLPC + 4 fixed-LPC candidates per
// frame in handle scratch) and the stand-alone controller kernel (frame_decide.cpp).
int encode_general_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const QlpcKernelArgs& a,
                          FrameDecideArgs& d, hipStream_t s) {
  const size_t n_sub = a.n_subframes, cstride = padded_stride(a.block_size);
  int rc;
  if (cfg->use_lpc) {
    LpcScratch lpc;
    if ((rc = lpc_scratch(h, n_sub, a.block_size, true, &lpc)) != FLACENC_HIP_OK) return rc;
    bool placed_lr = false;
    rc = enqueue(h, &cfg->qlpc, a.samples, n_sub, a.block_size, a.stride, nullptr, lpc.params, lpc.rows, cstride, nullptr,
                 nullptr, s, true, a.bps_uniform, a.residual, a.residual_stride, lpc.minmax, &placed_lr);
    if (rc != FLACENC_HIP_OK) return rc;
    d.lpc_lr_in_place = placed_lr ? 1u : 0u;
    d.minmax = placed_lr ? lpc.minmax : nullptr;
    d.lpc_params = lpc.params;
    d.lpc_residual = lpc.rows;
  }
  if (cfg->use_fixed) {
    FixedScratch fixed;
    if ((rc = fixed_scratch(h, n_sub, a.block_size, &fixed)) != FLACENC_HIP_OK) return rc;
    rc = enqueue_fixed(h, cfg, a.samples, n_sub, a.block_size, a.stride, nullptr, a.bps_uniform, true, fixed.params,
                       fixed.rows, cstride, fixed.keys, s);
    if (rc != FLACENC_HIP_OK) return rc;
    d.fixed_params = fixed.params;
    d.fixed_residual = fixed.rows;
    d.fixed_keys = fixed.keys;
  }
  HIP_TRY(h, launch_frame_decide(d, s));
  return FLACENC_HIP_OK;
}

// `pack` non-null: if the launch can run as the fused kernel with the bit writer, the frames are
// packed there (*packed = true, `residual` untouched); otherwise *packed = false and the call
// behaves like flacenc_hip_encode_stereo_frames_async (the caller packs in a second launch).
int encode_stereo_frames_impl(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                              size_t n_frames, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                              flacenc_hip_stereo_frame_result* results, int32_t* residual, size_t residual_stride,
                              void* stream, const PackTarget* pack, bool* packed) {
  if (packed) *packed = false;
  if (!h || !cfg || (!results && n_frames)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (cfg->qlpc.flags & FLACENC_HIP_FLAG_WASTED_BITS)  // (never the fused bit writer: the caller packs)
    return encode_wasted(h, cfg, frames, n_frames, 0, block_size, stride, bits_per_sample, results, nullptr, residual,
                         residual_stride, stream);
  int rc = check_batch_args(h, &cfg->qlpc, frames, n_frames * 4, block_size, stride,
                            reinterpret_cast<flacenc_hip_subframe_params*>(results), residual, residual_stride, 1);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  if (bits_per_sample < 8 || bits_per_sample > 24) {
    h->last_error = "bits_per_sample must be in 8..=24";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const flacenc_hip_frame_config run_cfg = frame_config(h, cfg, block_size);
  cfg = &run_cfg;
  if (cfg->use_fixed && (rc = verify_fixed(h, cfg)) != FLACENC_HIP_OK) return rc;
  bool fixed_composite = false;  // partitions not whole lane groups: general path
  const uint32_t group_log2 = fixed_group_log2(cfg, &fixed_composite);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  QlpcKernelArgs a;
  if ((rc = frame_args(h, cfg, frames, n_frames * 4, block_size, stride, bits_per_sample, true, residual, residual_stride,
                       group_log2, &a)) != FLACENC_HIP_OK)
    return rc;
  a.stamps = h->stamps;
  a.frame_results = results;
  if (a.reference_order) {  // R[] of the reference-order pass
    if ((rc = attach_split_scratch(h, a, stream)) != FLACENC_HIP_OK) return rc;
    rc = attach_sumabs_scratch(h, a, a.use_fixed && a.fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT);
    if (rc != FLACENC_HIP_OK) return rc;
  }
  // One kernel or two?  Measured on MI355X (24576 frames, order 8): with the fixed-LPC candidate the fused
  // bit writer takes 1.80 ms against 1.13 + 0.63 ms for the deciding kernel followed by the stand-alone
  // packer; without it 1.62 against 0.72 + 0.63 ms.  The deciding kernels run at three workgroups per CU,
  // the fused one -- whose packing tail keeps two of four waves busy -- fits only two, so the two-launch
  // form is the default; FLACENC_HIP_FLAG_FUSED_PACK / _TWO_STAGE_PACK in cfg->qlpc.flags override it.
  bool want_fused = false;
  if (cfg->qlpc.flags & FLACENC_HIP_FLAG_FUSED_PACK) want_fused = true;
  if (cfg->qlpc.flags & FLACENC_HIP_FLAG_TWO_STAGE_PACK) want_fused = false;
  // FLACENC_HIP_FLAG_ORDER_SEARCH / _WINDOW_SEARCH / _ORDER_GUESS / _PRECISION_SEARCH: the candidate batches +
  // frame_decide_kernel for every shape (FUSED_PACK ignored)
  // FLACENC_HIP_FLAG_RICE_ESCAPE: the same, whatever the candidates -- the pass sits between the batches and the decision
  const bool order_search = (lpc_search(cfg->qlpc.flags) && cfg->use_lpc) || (cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE);
  if (pack && want_fused && !fixed_composite && !order_search && block_size == 4096 && wave_kernel_eligible(a)) {
    attach_fused_pack(a, pack, bits_per_sample);
    if (packed) *packed = a.pack_out != nullptr;
  }
  if (a.split_scratch == nullptr && certify_needs_scratch(a)) {  // (the fused bit writer is handed the reference's R[])
    if ((rc = attach_split_scratch(h, a, stream)) != FLACENC_HIP_OK) return rc;
  }
  if (wave_kernel_eligible(a) && !fixed_composite && !order_search)
    return launch_adaptive(h, a, plan_qlpc_launch(block_size, cfg->qlpc.lpc_order), s);
  if (!order_search && big_block_frames(cfg, a)) return encode_big_block_frames(h, cfg, a, s);
  FrameDecideArgs d{};
  d.frames = frames;
  d.stride = stride;
  d.block_size = block_size;
  d.n_frames = static_cast<uint32_t>(n_frames);
  d.bits_per_sample = bits_per_sample;
  d.use_constant = cfg->use_constant;
  d.use_fixed = cfg->use_fixed;
  d.use_lpc = cfg->use_lpc;
  d.use_leftside = cfg->use_leftside;
  d.use_rightside = cfg->use_rightside;
  d.use_midside = cfg->use_midside;
  d.cand_stride = padded_stride(block_size);
  d.results = results;
  d.residual = residual;
  d.residual_stride = residual_stride;
  if (block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && subwave_shape(block_size) && !order_search) {
    bool taken = false;
    rc = subwave_frames(h, cfg, a, &d, nullptr, s, &taken);
    if (rc != FLACENC_HIP_OK || taken) return rc;
  }
  return encode_general_frames(h, cfg, a, d, s);
}

}  // namespace

extern "C" {

int flacenc_hip_encode_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                    const int32_t* frames, size_t n_frames, uint32_t channels,
                                    uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                    flacenc_hip_channel_result* results, int32_t* residual,
                                    size_t residual_stride, void* stream) {
  if (!h || !cfg || (!results && n_frames) || channels < 1 || channels > 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (cfg->qlpc.flags & FLACENC_HIP_FLAG_WASTED_BITS)
    return encode_wasted(h, cfg, frames, n_frames, channels, block_size, stride, bits_per_sample, nullptr, results,
                         residual, residual_stride, stream);
  const size_t n_sub = n_frames * channels;
  int rc = check_batch_args(h, &cfg->qlpc, frames, n_sub, block_size, stride,
                            reinterpret_cast<flacenc_hip_subframe_params*>(results), residual, residual_stride, 1);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  if (bits_per_sample < 8 || bits_per_sample > 24) {
    h->last_error = "bits_per_sample must be in 8..=24";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (cfg->use_fixed && (rc = verify_fixed(h, cfg)) != FLACENC_HIP_OK) return rc;
  const flacenc_hip_frame_config run_cfg = frame_config(h, cfg, block_size);
  cfg = &run_cfg;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t cstride = padded_stride(block_size);
  ChannelDecideArgs d{};
  d.samples = frames;
  d.stride = stride;
  d.block_size = block_size;
  d.n_subframes = static_cast<uint32_t>(n_sub);
  d.bits_per_sample = bits_per_sample;
  d.use_constant = cfg->use_constant;
  d.use_fixed = cfg->use_fixed;
  d.use_lpc = cfg->use_lpc;
  d.cand_stride = cstride;
  d.results = results;
  d.residual = residual;
  d.residual_stride = residual_stride;
  // FLACENC_HIP_FLAG_ORDER_SEARCH / _WINDOW_SEARCH: the candidate batches + channel_decide_kernel for every shape
  // ... and FLACENC_HIP_FLAG_RICE_ESCAPE, whose pass sits between the batches and the decision
  if (!((lpc_search(cfg->qlpc.flags) && cfg->use_lpc) || (cfg->qlpc.flags & FLACENC_HIP_FLAG_RICE_ESCAPE))) {
    // block size 4096, order <= 12: one fused kernel, a wave per channel (analysis, fixed-LPC
    // candidate, encode_subframe's choice, only the chosen residual written)
    bool composite = false;
    const uint32_t glog = fixed_group_log2(cfg, &composite);
    QlpcKernelArgs a;
    if ((rc = frame_args(h, cfg, frames, n_sub, block_size, stride, bits_per_sample, false, residual, residual_stride,
                         glog, &a)) != FLACENC_HIP_OK)
      return rc;
    a.chan_results = results;
    if (a.reference_order || certify_needs_scratch(a)) {  // R[] of the reference-order pass
      if ((rc = attach_split_scratch(h, a, stream)) != FLACENC_HIP_OK) return rc;
    }
    if ((rc = attach_sumabs_scratch(h, a, cfg->use_fixed && cfg->fixed_order_sel == FLACENC_HIP_ORDERSEL_APPROXENT)) !=
        FLACENC_HIP_OK)
      return rc;
    if (!composite && wave_kernel_eligible(a)) {
      QlpcLaunchPlan plan = plan_qlpc_launch(block_size, cfg->qlpc.lpc_order);
      return launch_adaptive(h, a, plan, s);
    }
    // the sub-wave kernel's independent-channel variant; what it marks takes the general path below, restricted to
    // the marked subframes
    if (block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && subwave_shape(block_size)) {
      bool taken = false;
      rc = subwave_frames(h, cfg, a, nullptr, &d, s, &taken);
      if (rc != FLACENC_HIP_OK || taken) return rc;
    }
  }
  if (cfg->use_lpc) {
    LpcScratch lpc;
    if ((rc = lpc_scratch(h, n_sub, block_size, false, &lpc)) != FLACENC_HIP_OK) return rc;
    rc = enqueue(h, &cfg->qlpc, frames, n_sub, block_size, stride, nullptr, lpc.params, lpc.rows, cstride, nullptr,
                 nullptr, s, false, bits_per_sample);
    if (rc != FLACENC_HIP_OK) return rc;
    d.lpc_params = lpc.params;
    d.lpc_residual = lpc.rows;
  }
  if (cfg->use_fixed) {
    FixedScratch fixed;
    if ((rc = fixed_scratch(h, n_sub, block_size, &fixed)) != FLACENC_HIP_OK) return rc;
    rc = enqueue_fixed(h, cfg, frames, n_sub, block_size, stride, nullptr, bits_per_sample, false, fixed.params,
                       fixed.rows, cstride, fixed.keys, s);
    if (rc != FLACENC_HIP_OK) return rc;
    d.fixed_params = fixed.params;
    d.fixed_residual = fixed.rows;
    d.fixed_keys = fixed.keys;
  }
  HIP_TRY(h, launch_channel_decide(d, s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_encode_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                              const int32_t* frames, size_t n_frames, uint32_t channels, uint32_t block_size,
                              size_t stride, uint32_t bits_per_sample, flacenc_hip_channel_result* results,
                              int32_t* residual, size_t residual_stride, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, flacenc_hip_encode_frames_async(h, cfg, frames, n_frames, channels, block_size, stride,
                                                      bits_per_sample, results, residual, residual_stride, h->stream),
                   n_frames == 0);
  if (memory_kind != FLACENC_HIP_MEM_HOST || !cfg || channels < 1 || channels > 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const size_t n_sub = n_frames * channels;
  int rc = check_batch_args(h, &cfg->qlpc, frames, n_sub, block_size, stride,
                            reinterpret_cast<flacenc_hip_subframe_params*>(results), residual, residual_stride, 1);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t dstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_samples, n_sub * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_sub * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_results, n_sub * sizeof(flacenc_hip_channel_result))) != FLACENC_HIP_OK) return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, frames, stride, block_size, n_sub)) != FLACENC_HIP_OK) return rc;
  rc = flacenc_hip_encode_frames_async(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), n_frames, channels,
                                       block_size, dstride, bits_per_sample,
                                       static_cast<flacenc_hip_channel_result*>(h->d_results.ptr),
                                       static_cast<int32_t*>(h->d_residual.ptr), dstride, s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, residual, residual_stride, h->d_residual, block_size, n_sub)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(results, h->d_results.ptr, n_sub * sizeof(flacenc_hip_channel_result),
                            hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

int flacenc_hip_encode_pack_stereo_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                                const int32_t* frames, size_t n_frames, uint32_t block_size,
                                                size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                                uint32_t first_frame_number, uint32_t frame_number_step,
                                                flacenc_hip_stereo_frame_result* results, uint8_t* out,
                                                size_t out_stride, uint32_t* out_len, void* stream) {
  if (!h || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (!out || !out_len || (reinterpret_cast<uintptr_t>(out) & 15) || (out_stride & 15) ||
      out_stride < flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample)) {
    h->last_error = "encode_pack_stereo_frames: out must be 16-byte aligned, out_stride a multiple of 16 and at least "
                    "flacenc_hip_stereo_frame_bytes_bound";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  const unsigned long long last = static_cast<unsigned long long>(first_frame_number) +
                                  static_cast<unsigned long long>(n_frames - 1) * frame_number_step;
  if (last >= (1ull << 31)) {
    h->last_error = "encode_pack_stereo_frames: frame_number must be below 2^31";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  // residual rows are only an intermediate here: handle scratch
  int rc;
  const size_t cstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_presid, n_frames * 2 * cstride * 4)) != FLACENC_HIP_OK) return rc;
  PackTarget pt;
  pt.out = out;
  pt.out_stride = out_stride;
  pt.out_len = out_len;
  pt.sample_rate = sample_rate;
  pt.first_frame_number = first_frame_number;
  pt.frame_number_step = frame_number_step;
  bool packed = false;
  rc = encode_stereo_frames_impl(h, cfg, frames, n_frames, block_size, stride, bits_per_sample, results,
                                 static_cast<int32_t*>(h->d_presid.ptr), cstride, stream, &pt, &packed);
  if (rc != FLACENC_HIP_OK || packed) return rc;
  return flacenc_hip_pack_stereo_frames_async(h, frames, n_frames, block_size, stride, results,
                                              static_cast<const int32_t*>(h->d_presid.ptr), cstride, bits_per_sample,
                                              sample_rate, first_frame_number, frame_number_step, out, out_stride,
                                              out_len, stream);
}

int flacenc_hip_encode_pack_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                         const int32_t* frames, size_t n_frames, uint32_t channels,
                                         uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                         uint32_t sample_rate, uint32_t first_frame_number,
                                         uint32_t frame_number_step, flacenc_hip_channel_result* results,
                                         uint8_t* out, size_t out_stride, uint32_t* out_len, void* stream) {
  if (!h || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return FLACENC_HIP_OK;
  if (channels < 1 || channels > 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  // residual rows are only an intermediate here: handle scratch
  int rc;
  const size_t cstride = padded_stride(block_size);
  if ((rc = ensure(h, h->d_presid, n_frames * channels * cstride * 4)) != FLACENC_HIP_OK) return rc;
  rc = flacenc_hip_encode_frames_async(h, cfg, frames, n_frames, channels, block_size, stride, bits_per_sample, results,
                                       static_cast<int32_t*>(h->d_presid.ptr), cstride, stream);
  if (rc != FLACENC_HIP_OK) return rc;
  return flacenc_hip_pack_frames_async(h, frames, n_frames, channels, block_size, stride, results,
                                       static_cast<const int32_t*>(h->d_presid.ptr), cstride, bits_per_sample,
                                       sample_rate, first_frame_number, frame_number_step, out, out_stride, out_len,
                                       stream);
}

int flacenc_hip_encode_stereo_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                           const int32_t* frames, size_t n_frames, uint32_t block_size,
                                           size_t stride, uint32_t bits_per_sample,
                                           flacenc_hip_stereo_frame_result* results, int32_t* residual,
                                           size_t residual_stride, void* stream) {
  return encode_stereo_frames_impl(h, cfg, frames, n_frames, block_size, stride, bits_per_sample, results, residual,
                                   residual_stride, stream, nullptr, nullptr);
}

int flacenc_hip_encode_stereo_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                     const int32_t* frames, size_t n_frames, uint32_t block_size,
                                     size_t stride, uint32_t bits_per_sample,
                                     flacenc_hip_stereo_frame_result* results, int32_t* residual,
                                     size_t residual_stride, int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (memory_kind == FLACENC_HIP_MEM_DEVICE)
    return drained(h, flacenc_hip_encode_stereo_frames_async(h, cfg, frames, n_frames, block_size, stride, bits_per_sample,
                                                             results, residual, residual_stride, h->stream),
                   n_frames == 0);
  if (memory_kind != FLACENC_HIP_MEM_HOST || !cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_frames == 0) return flacenc_hip_verify_config(&cfg->qlpc);
  if (!frames || !results || !residual) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t dstride = padded_stride(block_size);
  int rc;
  if ((rc = ensure(h, h->d_samples, n_frames * 2 * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_residual, n_frames * 2 * dstride * 4)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_params, n_frames * sizeof(flacenc_hip_stereo_frame_result))) != FLACENC_HIP_OK)
    return rc;
  hipStream_t s = h->stream;
  if ((rc = rows_to_device(h, h->d_samples, frames, stride, block_size, n_frames * 2)) != FLACENC_HIP_OK) return rc;
  rc = flacenc_hip_encode_stereo_frames_async(h, cfg, static_cast<const int32_t*>(h->d_samples.ptr), n_frames,
                                              block_size, dstride, bits_per_sample,
                                              static_cast<flacenc_hip_stereo_frame_result*>(h->d_params.ptr),
                                              static_cast<int32_t*>(h->d_residual.ptr), dstride, s);
  if (rc != FLACENC_HIP_OK) return rc;
  if ((rc = rows_to_host(h, residual, residual_stride, h->d_residual, block_size, n_frames * 2)) != FLACENC_HIP_OK) return rc;
  HIP_TRY(h, hipMemcpyAsync(results, h->d_params.ptr, n_frames * sizeof(flacenc_hip_stereo_frame_result),
                            hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return FLACENC_HIP_OK;
}

}  // extern "C"
