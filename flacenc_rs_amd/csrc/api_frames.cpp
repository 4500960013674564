// api_frames.cpp -- encode_frame's decisions for batches of frames: Independent(channels) frames, 2-channel frames with
// the stereo decision (both: check, plan_frame_call, run_frame_plan), FLACENC_HIP_FLAG_WASTED_BITS around them, encode + pack.
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
int encode_frames_common(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames, size_t n_frames,
                         uint32_t channels, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                         flacenc_hip_stereo_frame_result* results, flacenc_hip_channel_result* chan_results,
                         int32_t* residual, size_t residual_stride, void* stream, const PackTarget* pack, bool* packed);

// The general path's candidates (what flacenc_hip_qlpc_batch and flacenc_hip_fixed_lpc_batch run) in handle scratch, for
// the stereo call (with the roles' min / max), the Independent(n) call, the big-block form and the wasted-bits fix-up
int enqueue_candidates(flacenc_hip_handle* h, const flacenc_hip_frame_config& cfg, bool lpc_batch, bool fixed_batch,
                       const CandidateBatch& rows, hipStream_t s, Candidates* out) {
  const size_t cstride = padded_stride(rows.block_size);
  int rc;
  if ((rc = candidate_scratch(h, rows.n_subframes, rows.block_size, lpc_batch, fixed_batch, rows.stereo, out)) != FLACENC_HIP_OK)
    return rc;
  if (lpc_batch) {
    CandidateBatch b = rows;
    b.write_to(out->lpc_params, out->lpc_residual, cstride);
    b.minmax_out = out->minmax;
    if ((rc = enqueue(h, &cfg.qlpc, b, s)) != FLACENC_HIP_OK) return rc;
    out->placed = b.placed;
  }
  if (fixed_batch) {
    CandidateBatch b = rows;
    b.write_to(out->fixed_params, out->fixed_residual, cstride);
    b.selector_keys = out->fixed_keys;
    if ((rc = enqueue_fixed(h, &cfg, b, s)) != FLACENC_HIP_OK) return rc;
  }
  return FLACENC_HIP_OK;
}
// (the deciding kernels' records -- FrameDecideArgs, ChannelDecideArgs, WastedArgs -- name the candidates alike)
template <typename Decide>
void name_candidates(Decide& d, const Candidates& c) {
  d.lpc_params = c.lpc_params;
  d.lpc_residual = c.lpc_residual;
  d.fixed_params = c.fixed_params;
  d.fixed_residual = c.fixed_residual;
  d.fixed_keys = c.fixed_keys;
}
// qlpc_subwave_kernel's frame variants on blocks of 8 / 16 / 32 finest Rice partitions (512 .. 2304 samples), and the
// clean-up of what they marked.  The kernel does the whole of encode_frame (`fd`: 2-channel frames, both candidates of
// the four roles, the decision, the two chosen rows) resp. encode_subframe of every channel (`cd`: independent
// channels) in one launch, several frames per workgroup.  A frame (a subframe) with a candidate beyond its exact sums
// (residuals of 2^25 and more) comes back marked and takes the general path, restricted to what is marked: the QLPC
// clean-up, the fixed_lpc clean-up and the deciding kernel, three launches that return at once when the count is 0.
// Exactly one of `fd` / `cd` is given, filled but for the candidates.  A plan on another path than kSubwave: the split
// scratch is attached all the same, nothing is launched.
int subwave_frames(flacenc_hip_handle* h, const FramePlan& p, const QlpcKernelArgs& a, FrameDecideArgs* fd,
                   ChannelDecideArgs* cd, hipStream_t s) {
  int rc;
  QlpcKernelArgs m = a;
  subwave_fields(m, p.cfg, p.cert_subwave);
  if ((rc = attach_scratch(h, m, scratch_grant(m, LaunchKind::kSubwaveFrames), s)) != FLACENC_HIP_OK) return rc;
  m.marked_unit = fd ? 4 : 1;  // (the frame variant lists marked FRAMES; the candidate clean-ups visit their four roles)
  if (p.path != FramePlan::kSubwave) return FLACENC_HIP_OK;
  Candidates cand;
  if ((rc = candidate_scratch(h, a.n_subframes, a.block_size, true, p.cfg.use_fixed, false, &cand)) != FLACENC_HIP_OK) return rc;
  m.cand_lpc_params = cand.lpc_params;
  m.cand_fixed_params = cand.fixed_params;
  HIP_TRY(h, launch_subwave_frames(m, s));
  // the marked candidates, by the generic kernel's clean-up launches (status -1 in the scratch records)
  QlpcKernelArgs c = m;
  c.frame_results = nullptr;
  c.chan_results = nullptr;
  c.cand_lpc_params = c.cand_fixed_params = nullptr;
  c.params = cand.lpc_params;
  c.residual = cand.lpc_residual;
  c.residual_stride = padded_stride(a.block_size);
  c.only_marked = 1;
  c.use_fixed = 0;
  c.fixed_keys = nullptr;
  HIP_TRY(h, launch_qlpc(c, plan_qlpc_launch(a.block_size, p.cfg.qlpc.lpc_order), s));
  if (p.cfg.use_fixed) {
    QlpcKernelArgs x = c;
    x.params = cand.fixed_params;
    x.residual = cand.fixed_residual;
    x.selector_keys = cand.fixed_keys;
    x.window = nullptr;
    x.window_lanes = nullptr;
    x.flat_lo = x.flat_hi = 0;
    fixed_batch_fields(x, p.cfg);
    HIP_TRY(h, launch_qlpc(x, plan_qlpc_launch(a.block_size, 4), s));
  }
  // (the two deciding kernels' records name the candidates and the marked list alike; entries: frames resp. subframes)
  auto marked_candidates = [&](auto& d) {
    name_candidates(d, cand);
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
// kernel that writes their records and residual rows over the first pass's.  Device pointers, `stream`; checked arguments.
int encode_wasted(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames, size_t n_frames,
                  uint32_t channels, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                  flacenc_hip_stereo_frame_result* results, flacenc_hip_channel_result* chan_results, int32_t* residual,
                  size_t residual_stride, void* stream) {
  const bool stereo = channels == 0;
  const size_t rows = stereo ? 4 : channels;
  int rc;
  // the unflagged configuration (FUSED_PACK: a kernel choice the fix-up's packer has no part in)
  flacenc_hip_frame_config plain = *cfg;
  plain.qlpc.flags = search_flags(!h->lpc_windows.empty(), h->precision_floor, cfg->qlpc.flags, cfg->qlpc.quant_precision) &
                     ~(FLACENC_HIP_FLAG_WASTED_BITS | FLACENC_HIP_FLAG_FUSED_PACK);
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
    rc = encode_frames_common(h, &plain, frames, n_frames, channels, block_size, stride, bits_per_sample, results,
                              chan_results, residual, residual_stride, stream, nullptr, nullptr);
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
  // estimated_qlpc and fixed_lpc of the shifted rows, each at its own width
  CandidateBatch shifted(w.shifted, n_rows, block_size, cstride, w.shifted_bps);
  Candidates cand;
  if ((rc = enqueue_candidates(h, plain, plain.use_lpc, plain.use_fixed, shifted, s, &cand)) != FLACENC_HIP_OK) return rc;
  name_candidates(w, cand);
  HIP_TRY(h, launch_wasted_decide(w, s));
  return FLACENC_HIP_OK;
}

// Frame::write inside the deciding wave kernel: the header constants and CRC powers of `pack` into the launch record.
// The frame's bit buffer reuses the two channel images; FrameCall::pack says whether it fits there (at most 35424 bytes).
uint32_t pack_lds_words(uint32_t block_size, uint32_t bits_per_sample) {
  return static_cast<uint32_t>(flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample) / 4 + 4);
}
void attach_fused_pack(QlpcKernelArgs& a, const PackTarget* pack, uint32_t bits_per_sample) {
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
  a.pack_lds_words = pack_lds_words(a.block_size, bits_per_sample);
  fill_crc_powers(a.pack_lds_words, &a.pack_crc_per, a.pack_crc_pow);
}

// Runs a plan, in its order: the frame-level record with its scratch; the fused kernel, or the big-block form, or the
// sub-wave kernel with the general path behind it for what it marked, or the general path -- the candidate batches (4 QLPC
// + 4 fixed-LPC candidates per frame in handle scratch) and the stand-alone deciding kernel (frame_decide.cpp).
int run_frame_plan(flacenc_hip_handle* h, const FrameCall& c, const FramePlan& p, size_t n_frames, uint32_t channels,
                   flacenc_hip_stereo_frame_result* results, flacenc_hip_channel_result* chan_results, int32_t* residual,
                   const PackTarget* pack, hipStream_t s) {
  const flacenc_hip_frame_config& cfg = p.cfg;
  const size_t n_sub = n_frames * (c.stereo ? 4 : channels);
  int rc;
  QlpcKernelArgs a;
  if (p.frame_record) {
    // base_args with the config's window (none for a short block, which never reads it: short blocks take the
    // candidate-free general path), the output rows and encode_frame's switches
    const WindowEntry* win = nullptr;
    if (c.block_size >= FLACENC_HIP_MIN_BLOCK_SIZE && (rc = get_window(h, &cfg.qlpc, c.block_size, &win)) != FLACENC_HIP_OK) return rc;
    a = base_args(h, cfg.qlpc, win, c.samples, c.stride, c.block_size, n_sub, nullptr, c.bits_per_sample, c.stereo);
    a.residual = residual;
    a.residual_stride = c.residual_stride;
    frame_fields(a, cfg, c.stereo, p.group_log2);
    a.fixed_keys = h->fixed_keys;
    if (c.stereo) a.stamps = h->stamps;
    a.frame_results = results;
    a.chan_results = chan_results;
    // One kernel or two?  Measured on MI355X (24576 frames, order 8): with the fixed-LPC candidate the fused
    // bit writer takes 1.80 ms against 1.13 + 0.63 ms for the deciding kernel followed by the stand-alone
    // packer; without it 1.62 against 0.72 + 0.63 ms.  The deciding kernels run at three workgroups per CU,
    // the fused one -- whose packing tail keeps two of four waves busy -- fits only two, so the two-launch
    // form is the default; FLACENC_HIP_FLAG_FUSED_PACK / _TWO_STAGE_PACK in cfg->qlpc.flags override it.
    if (p.fused_pack) attach_fused_pack(a, pack, c.bits_per_sample);
    if ((rc = attach_scratch(h, a, scratch_grant(a, LaunchKind::kFrame), s)) != FLACENC_HIP_OK) return rc;
  }
  // block size 4096 / 4608, order <= 12: one fused kernel (analysis, fixed-LPC candidate, the decision, only the chosen
  // residual written; Independent(n): a wave per channel)
  if (p.path == FramePlan::kFused) return launch_adaptive(h, a, plan_qlpc_launch(c.block_size, cfg.qlpc.lpc_order), s);
  CandidateBatch rows(c.samples, n_sub, c.block_size, c.stride);
  rows.bps_uniform = c.bits_per_sample;
  rows.stereo = c.stereo;
  Candidates cand;
  if (p.path == FramePlan::kBigBlock) {
    // Big-block shapes: two analyse-only passes (QLPC, fixed_lpc: records, no residual rows), then one kernel that
    // decides and writes only the two rows the frame keeps (bigblock_residual_kernel, modes 1 and 2) -- eight candidate
    // rows per frame stay off HBM, and so does the copy of the chosen two.
    rows.analyse_only = true;
    if ((rc = enqueue_candidates(h, cfg, p.lpc_batch, p.fixed_batch, rows, s, &cand)) != FLACENC_HIP_OK) return rc;
    a.residual_mode = 2u;  // (shape, width, the frame's results and rows and the encode_frame switches are set)
    a.stamps = nullptr;
    a.cand_lpc_params = cand.lpc_params;
    a.cand_lpc_rows = cand.lpc_residual;
    a.cand_minmax = cand.minmax;
    a.cand_stride = padded_stride(c.block_size);
    a.cand_fixed_params = cand.fixed_params;
    a.cand_fixed_rows = cand.fixed_residual;
    a.cand_fixed_keys = cand.fixed_keys;
    HIP_TRY(h, launch_bigblock_residual(a, s));
    return FLACENC_HIP_OK;
  }
  FrameDecideArgs fd{};
  ChannelDecideArgs cd{};
  auto decide_fields = [&](auto& d) {
    d.stride = c.stride;
    d.block_size = c.block_size;
    d.bits_per_sample = c.bits_per_sample;
    d.use_constant = cfg.use_constant;
    d.use_fixed = cfg.use_fixed;
    d.use_lpc = cfg.use_lpc;
    d.cand_stride = padded_stride(c.block_size);
    d.residual = residual;
    d.residual_stride = c.residual_stride;
  };
  if (c.stereo) {
    decide_fields(fd);
    fd.frames = c.samples;
    fd.n_frames = static_cast<uint32_t>(n_frames);
    fd.use_leftside = cfg.use_leftside;
    fd.use_rightside = cfg.use_rightside;
    fd.use_midside = cfg.use_midside;
    fd.results = results;
  } else {
    decide_fields(cd);
    cd.samples = c.samples;
    cd.n_subframes = static_cast<uint32_t>(n_sub);
    cd.results = chan_results;
  }
  if (p.subwave_scratch) {
    rc = subwave_frames(h, p, a, c.stereo ? &fd : nullptr, c.stereo ? nullptr : &cd, s);
    if (rc != FLACENC_HIP_OK || p.path == FramePlan::kSubwave) return rc;
  }
  if (c.stereo) {  // (the big-block shapes: L / R in place)
    rows.residual_lr = residual;
    rows.residual_lr_stride = c.residual_stride;
  }
  if ((rc = enqueue_candidates(h, cfg, p.lpc_batch, p.fixed_batch, rows, s, &cand)) != FLACENC_HIP_OK) return rc;
  if (c.stereo) {
    name_candidates(fd, cand);
    fd.lpc_lr_in_place = cand.placed ? 1u : 0u;
    fd.minmax = cand.placed ? cand.minmax : nullptr;
    HIP_TRY(h, launch_frame_decide(fd, s));
  } else {
    name_candidates(cd, cand);
    HIP_TRY(h, launch_channel_decide(cd, s));
  }
  return FLACENC_HIP_OK;
}

// Both frame-level calls: check the arguments, plan, run the plan.  channels == 0: 2-channel frames into `results`, else
// Independent(channels) frames into `chan_results`.  `pack` non-null: if the launch can run as the fused kernel with the bit
// writer, the frames are packed there (*packed = true, `residual` untouched); otherwise the caller packs in a second launch.
int encode_frames_common(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames, size_t n_frames,
                         uint32_t channels, uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                         flacenc_hip_stereo_frame_result* results, flacenc_hip_channel_result* chan_results,
                         int32_t* residual, size_t residual_stride, void* stream, const PackTarget* pack, bool* packed) {
  if (packed) *packed = false;
  const bool stereo = channels == 0;
  void* const records = stereo ? static_cast<void*>(results) : static_cast<void*>(chan_results);
  if (!h || !cfg || (!records && n_frames)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  int rc = check_batch_args(h, &cfg->qlpc, frames, n_frames * (stereo ? 4 : channels), block_size, stride,
                            static_cast<flacenc_hip_subframe_params*>(records), residual, residual_stride, 1);
  if (rc != FLACENC_HIP_OK || n_frames == 0) return rc;
  if ((rc = check_bits_per_sample(h, bits_per_sample)) != FLACENC_HIP_OK) return rc;
  const bool wasted = (cfg->qlpc.flags & FLACENC_HIP_FLAG_WASTED_BITS) != 0;
  // (the plain stereo call has always let a short block's fixed config pass unverified: too_short drops it)
  const bool unverified = stereo && !wasted && block_size < FLACENC_HIP_MIN_BLOCK_SIZE;
  if (cfg->use_fixed && !unverified && (rc = verify_fixed(h, cfg)) != FLACENC_HIP_OK) return rc;
  if (wasted)  // (never the fused bit writer: the caller packs)
    return encode_wasted(h, cfg, frames, n_frames, channels, block_size, stride, bits_per_sample, results, chan_results,
                         residual, residual_stride, stream);
  const FrameCall call{*cfg, stereo, block_size, bits_per_sample, frames, stride, residual, residual_stride,
                       pack && pack_lds_words(block_size, bits_per_sample) * 4ull <= 35424, !h->lpc_windows.empty(), h->precision_floor};
  const FramePlan plan = plan_frame_call(call);
  HIP_TRY(h, hipSetDevice(h->device));
  if (packed) *packed = plan.fused_pack;
  return run_frame_plan(h, call, plan, n_frames, channels, results, chan_results, residual, pack, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int flacenc_hip_encode_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                    const int32_t* frames, size_t n_frames, uint32_t channels,
                                    uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                    flacenc_hip_channel_result* results, int32_t* residual,
                                    size_t residual_stride, void* stream) {
  if (channels < 1 || channels > 8) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  return encode_frames_common(h, cfg, frames, n_frames, channels, block_size, stride, bits_per_sample, nullptr, results,
                              residual, residual_stride, stream, nullptr, nullptr);
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
  const PackTarget pt{out, out_stride, out_len, sample_rate, first_frame_number, frame_number_step};
  bool packed = false;
  rc = encode_frames_common(h, cfg, frames, n_frames, 0, block_size, stride, bits_per_sample, results, nullptr,
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
  return encode_frames_common(h, cfg, frames, n_frames, 0, block_size, stride, bits_per_sample, results, nullptr, residual,
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
