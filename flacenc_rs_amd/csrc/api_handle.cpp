// api_handle.cpp -- the handle's life cycle, config verification, pinned memory and the helpers every unit uses.
#include <cstdio>
#include <new>

#include "api_internal.h"

namespace flacenc_hip {
CommState*& handle_comm_slot(flacenc_hip_handle* h) { return h->comm; }
int handle_device(const flacenc_hip_handle* h) { return h->device; }
void handle_set_error(flacenc_hip_handle* h, const std::string& what) { h->last_error = what; }

bool set_error(flacenc_hip_handle* h, const char* what, hipError_t err) {
  if (h) {
    char buf[512];
    std::snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(err));
    h->last_error = buf;
  }
  return false;
}

int ensure(flacenc_hip_handle* h, DeviceBuffer& b, size_t bytes) {
  if (bytes <= b.cap) return FLACENC_HIP_OK;
  if (b.ptr) HIP_TRY(h, hipFree(b.ptr));
  b.ptr = nullptr;
  b.cap = 0;
  size_t want = bytes + bytes / 4 + 256;
  HIP_TRY(h, hipMalloc(&b.ptr, want));
  b.cap = want;
  return FLACENC_HIP_OK;
}

std::vector<DeviceBuffer*> device_buffers(flacenc_hip_handle* h) {
  std::vector<DeviceBuffer*> all = {
      &h->d_samples, &h->d_residual, &h->d_params, &h->d_bps, &h->d_autocorr, &h->d_lpc, &h->d_tables, &h->d_keys, &h->d_sel,
      &h->d_results, &h->d_out, &h->d_outlen, &h->d_cparams, &h->d_cresid, &h->d_fparams, &h->d_fresid, &h->d_fkeys,
      &h->d_split, &h->d_presid, &h->d_sumabs, &h->d_minmax, &h->d_marked, &h->d_irlsw, &h->d_gram, &h->d_esc, &h->d_wide, &h->d_dec,
      &h->d_dec_io, &h->d_idx, &h->d_vbs_frames, &h->d_vbs_results, &h->d_vbs_pack, &h->d_vbs_meta, &h->d_vbs_io, &h->d_wk,
      &h->d_wlist, &h->d_wrows, &h->d_wbps, &h->d_order, &h->d_ppk_off, &h->d_ppk_io, &h->d_dpcm_idx, &h->d_md5, &h->d_encs};
  for (int i = 0; i < 2; ++i)
    for (DeviceBuffer* b : {&h->d_pcm[i], &h->d_pack[i], &h->d_plen[i], &h->d_poff[i], &h->d_cont[i]}) all.push_back(b);
  return all;
}

int drained(flacenc_hip_handle* h, int rc, bool nothing_queued) {
  if (rc != FLACENC_HIP_OK || nothing_queued) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLACENC_HIP_OK;
}

int rows_to_device(flacenc_hip_handle* h, const DeviceBuffer& b, const int32_t* rows, size_t stride, uint32_t block_size,
                   size_t n_rows) {
  HIP_TRY(h, hipMemcpy2DAsync(b.ptr, padded_stride(block_size) * 4, rows, stride * 4, static_cast<size_t>(block_size) * 4,
                              n_rows, hipMemcpyHostToDevice, h->stream));
  return FLACENC_HIP_OK;
}

int rows_to_host(flacenc_hip_handle* h, int32_t* rows, size_t stride, const DeviceBuffer& b, uint32_t block_size,
                 size_t n_rows) {
  HIP_TRY(h, hipMemcpy2DAsync(rows, stride * 4, b.ptr, padded_stride(block_size) * 4, static_cast<size_t>(block_size) * 4,
                              n_rows, hipMemcpyDeviceToHost, h->stream));
  return FLACENC_HIP_OK;
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" {

int flacenc_hip_abi_version(void) { return FLACENC_HIP_ABI_VERSION; }

int flacenc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int flacenc_hip_create(flacenc_hip_handle** out, int device_id) {
  if (!out) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FLACENC_HIP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  flacenc_hip_handle* h = new (std::nothrow) flacenc_hip_handle();
  if (!h) return FLACENC_HIP_ERR_DEVICE;
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return FLACENC_HIP_ERR_DEVICE;
  }
  *out = h;
  return FLACENC_HIP_OK;
}

void flacenc_hip_destroy(flacenc_hip_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  flacenc_hip::comm_release(h->comm);
  h->comm = nullptr;
  for (WindowEntry& e : h->windows)
    if (e.dev) (void)hipFree(e.dev);
  for (DeviceBuffer* b : device_buffers(h))
    if (b->ptr) (void)hipFree(b->ptr);
  if (h->adaptive.d_counters) (void)hipFree(h->adaptive.d_counters);  // (the order mode's counters and their pinned mirror)
  if (h->adaptive.verdict) (void)hipHostFree(h->adaptive.verdict);
  for (int i = 0; i < 2; ++i) {
    for (void* p : {h->pin_in[i], h->pin_out[i], h->pin_meta[i]})
      if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {h->ev_h2d[i], h->ev_fill[i], h->ev_pack[i], h->ev_d2h[i]})
      if (e) (void)hipEventDestroy(e);
  }
  if (h->s_in) (void)hipStreamDestroy(h->s_in);
  if (h->s_out) (void)hipStreamDestroy(h->s_out);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char* flacenc_hip_last_error(const flacenc_hip_handle* h) {
  return h ? h->last_error.c_str() : "null handle";
}

int flacenc_hip_verify_config(const flacenc_hip_qlpc_config* cfg) {
  if (!cfg) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  const uint32_t max_order = (cfg->flags & FLACENC_HIP_FLAG_ALLOW_ORDER_32)
                                 ? FLACENC_HIP_MAX_LPC_ORDER
                                 : FLACENC_HIP_REF_MAX_LPC_ORDER;
  // config::Qlpc::verify, src/config.rs:302-326
  if (cfg->lpc_order < 1 || cfg->lpc_order > max_order) return FLACENC_HIP_ERR_BAD_CONFIG;
  if (cfg->quant_precision < 1 || cfg->quant_precision > FLACENC_HIP_MAX_PRECISION)
    return FLACENC_HIP_ERR_BAD_CONFIG;
  // config::Window::verify, src/config.rs:371-387
  if (cfg->window_type == FLACENC_HIP_WINDOW_TUKEY) {
    if (!(cfg->tukey_alpha >= 0.0f && cfg->tukey_alpha <= 1.0f)) return FLACENC_HIP_ERR_BAD_CONFIG;
  } else if (cfg->window_type != FLACENC_HIP_WINDOW_RECTANGLE) {
    return FLACENC_HIP_ERR_BAD_CONFIG;
  }
  // config::Prc::verify, src/config.rs:224-229
  if (cfg->max_rice_parameter > FLACENC_HIP_MAX_RICE_PARAMETER) return FLACENC_HIP_ERR_BAD_CONFIG;
  // config::Qlpc::use_direct_mse / mae_optimization_steps (src/config.rs:280-285): accepted as in the
  // reference's `experimental` build
  if (cfg->use_direct_mse > 1 || cfg->mae_optimization_steps > FLACENC_HIP_MAX_MAE_STEPS) return FLACENC_HIP_ERR_BAD_CONFIG;
  // one summation order at a time; the simd-nightly order is only defined up to lag 15 (beyond, `as_simd`
  // splits 128- and 256-byte vectors at addresses the allocator picks, src/lpc.rs:459, :519-523)
  if ((cfg->flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER) && (cfg->flags & FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER))
    return FLACENC_HIP_ERR_BAD_CONFIG;
  if ((cfg->flags & FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER) && cfg->lpc_order > 15) return FLACENC_HIP_ERR_UNSUPPORTED;
  // the order search runs on the autocorrelation's R[]; the covariance-method estimator has none
  if ((cfg->flags & FLACENC_HIP_FLAG_ORDER_SEARCH) && cfg->use_direct_mse) return FLACENC_HIP_ERR_UNSUPPORTED;
  if ((cfg->flags & FLACENC_HIP_FLAG_WINDOW_SEARCH) && cfg->use_direct_mse) return FLACENC_HIP_ERR_UNSUPPORTED;
  // the guessed search is a subset of the exhaustive one: one of the two at a time
  if ((cfg->flags & FLACENC_HIP_FLAG_ORDER_GUESS) && (cfg->flags & FLACENC_HIP_FLAG_ORDER_SEARCH)) return FLACENC_HIP_ERR_BAD_CONFIG;
  if ((cfg->flags & FLACENC_HIP_FLAG_ORDER_GUESS) && cfg->use_direct_mse) return FLACENC_HIP_ERR_UNSUPPORTED;
  // the precision search requantises the recursion's coefficients: a third axis of the same search
  if ((cfg->flags & FLACENC_HIP_FLAG_PRECISION_SEARCH) && cfg->use_direct_mse) return FLACENC_HIP_ERR_UNSUPPORTED;
  return FLACENC_HIP_OK;
}

int flacenc_hip_set_order_guesses(flacenc_hip_handle* h, uint32_t k) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (k < 1 || k > 32) {
    h->last_error = "flacenc_hip_set_order_guesses: k must be in 1..=32";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->order_guesses = k;
  return FLACENC_HIP_OK;
}

int flacenc_hip_set_precision_floor(flacenc_hip_handle* h, uint32_t floor) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (floor < 1 || floor > FLACENC_HIP_MAX_PRECISION) {
    h->last_error = "flacenc_hip_set_precision_floor: floor must be in 1..=15";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->precision_floor = floor;
  return FLACENC_HIP_OK;
}

int flacenc_hip_set_max_bits_per_sample(flacenc_hip_handle* h, uint32_t bits) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (bits != 24 && bits != 32) {
    h->last_error = "flacenc_hip_set_max_bits_per_sample: bits must be 24 or 32";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->max_bps = bits;
  return FLACENC_HIP_OK;
}

int flacenc_hip_set_max_encode_bits_per_sample(flacenc_hip_handle* h, uint32_t bits) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (bits != 24 && bits != 32) {
    h->last_error = "flacenc_hip_set_max_encode_bits_per_sample: bits must be 24 or 32";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  h->max_encode_bps = bits;
  return FLACENC_HIP_OK;
}

void* flacenc_hip_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void flacenc_hip_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int flacenc_hip_set_host_threads(flacenc_hip_handle* h, int threads) {
  if (!h || threads < 0 || threads > 64) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  h->host_threads = threads;
  h->copy_pool.reset();  // rebuilt with the new size at the next pageable call
  return FLACENC_HIP_OK;
}

int flacenc_hip_synchronize(flacenc_hip_handle* h) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLACENC_HIP_OK;
}

}  // extern "C"
