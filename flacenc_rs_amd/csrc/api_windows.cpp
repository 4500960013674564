// api_windows.cpp -- the analysis windows: the reference's weights, the window search's pieces and the handle's cache
// of them on the device.
#include <cmath>

#include "api_internal.h"
#include "window_lanes_core.h"

namespace flacenc_hip {
namespace {

// lpc::window_weights, src/lpc.rs:96-120: f32 arithmetic in exactly this order,
// libm cosf (what f32::cos lowers to on Linux).  Built with -ffp-contract=off.
void window_weights(uint32_t type, float alpha, size_t len, float* out) {
  if (type == FLACENC_HIP_WINDOW_RECTANGLE || alpha == 0.0f) {
    for (size_t t = 0; t < len; ++t) out[t] = 1.0f;
    return;
  }
  const float pi = 3.14159265358979323846f;
  const float max_t = static_cast<float>(len) - 1.0f;
  const float alpha_len = alpha * max_t;
  for (size_t ti = 0; ti < len; ++ti) {
    const float t = static_cast<float>(ti);
    float w;
    if (t < alpha_len / 2.0f) {
      const float arg = 2.0f * pi * t / alpha_len;
      w = 0.5f * (1.0f - cosf(arg));
    } else if (t < max_t - alpha_len / 2.0f) {
      w = 1.0f;
    } else {
      const float arg = 2.0f * pi * (max_t - t) / alpha_len;
      w = 0.5f * (1.0f - cosf(arg));
    }
    out[ti] = w;
  }
}

// T(m), the reference's Tukey weights of length m (lpc::window_weights); all zeros below 2 samples, where the reference's
// formula gives NaN
void tukey_piece(float alpha, size_t m, float* out) {
  if (m < 2) {
    for (size_t t = 0; t < m; ++t) out[t] = 0.0f;
    return;
  }
  window_weights(FLACENC_HIP_WINDOW_TUKEY, alpha, m, out);
}

// An analysis window of FLACENC_HIP_FLAG_WINDOW_SEARCH over a block of n samples: s = (start n) >> 16, e = (end n) >> 16
// (64-bit integers, no floating point), RECTANGLE all ones, TUKEY T(n), PARTIAL_TUKEY T(e - s) on [s, e) and zeros
// elsewhere, PUNCHOUT_TUKEY T(s) on [0, s), zeros on [s, e), T(n - e) on [e, n).
void lpc_window_weights(uint32_t type, float alpha, uint32_t start, uint32_t end, size_t n, float* out) {
  if (type == FLACENC_HIP_WINDOW_RECTANGLE) {
    window_weights(type, alpha, n, out);
    return;
  }
  if (type == FLACENC_HIP_WINDOW_TUKEY) {
    tukey_piece(alpha, n, out);
    return;
  }
  const size_t s = static_cast<size_t>((static_cast<uint64_t>(start) * n) >> 16);
  const size_t e = static_cast<size_t>((static_cast<uint64_t>(end) * n) >> 16);
  for (size_t t = 0; t < n; ++t) out[t] = 0.0f;
  if (type == FLACENC_HIP_WINDOW_PARTIAL_TUKEY) {
    tukey_piece(alpha, e - s, out + s);
  } else {
    tukey_piece(alpha, s, out);
    tukey_piece(alpha, n - e, out + e);
  }
}

// flacenc_hip_set_lpc_windows / flacenc_hip_lpc_window_weights: an entry's validity
bool lpc_window_ok(uint32_t type, float alpha, uint32_t start, uint32_t end) {
  if (type > FLACENC_HIP_WINDOW_PUNCHOUT_TUKEY) return false;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return false;  // (NaN included)
  if (type >= FLACENC_HIP_WINDOW_PARTIAL_TUKEY && (start >= end || end > FLACENC_HIP_WINDOW_UNIT)) return false;
  return true;
}

}  // namespace

// get_window, src/lpc.rs:222-231.  The reference keys its cache by
// (size, fingerprint) where the fingerprint quantises alpha to 16 bits
// (src/lpc.rs:123-132), so two alphas closer than 1/65535 share the first
// one's table; this cache keys by the exact alpha bits instead (and by the
// piece of the window search's partial / punch-out windows).  Entries stay
// until flacenc_hip_destroy: a queued launch may still read any of them.
int get_window_entry(flacenc_hip_handle* h, uint32_t type, float alpha, uint32_t start, uint32_t end, uint32_t n,
                     const WindowEntry** out) {
  uint32_t alpha_bits;
  std::memcpy(&alpha_bits, &alpha, 4);
  if (type == FLACENC_HIP_WINDOW_TUKEY && alpha == 0.0f) type = FLACENC_HIP_WINDOW_RECTANGLE;
  if (type == FLACENC_HIP_WINDOW_RECTANGLE) alpha_bits = 0;
  if (type < FLACENC_HIP_WINDOW_PARTIAL_TUKEY) start = end = 0;
  for (const WindowEntry& e : h->windows) {
    if (e.n == n && e.type == type && e.alpha_bits == alpha_bits && e.start == start && e.end == end) {
      *out = &e;
      return FLACENC_HIP_OK;
    }
  }
  WindowEntry e;
  e.n = n;
  e.type = type;
  e.alpha_bits = alpha_bits;
  e.start = start;
  e.end = end;
  e.dev = nullptr;
  e.dev_lanes = nullptr;
  e.flat_lo = -64;
  e.flat_hi = 0x7FFFFFFF;
  if (type != FLACENC_HIP_WINDOW_RECTANGLE) {
    const size_t rows = (n + 15) / 16;
    const size_t total = 32 + rows * 16 + 16;
    // blocks of 4096: the lane-major copy the fused kernel reads (window_lanes_core.h) follows in the same allocation and
    // the same upload, 256-byte aligned
    const size_t lanes_at = n == window_lanes::kBlock ? ((total + 63) & ~static_cast<size_t>(63)) : 0;
    std::vector<float> host(lanes_at ? lanes_at + window_lanes::kFloats : total, 0.0f);
    lpc_window_weights(type, alpha, start, end, n, host.data() + 32);
    // longest run of exactly-1.0 weights: chunks inside it skip the table
    int best_lo = 0, best_hi = 0, run_lo = -1;
    for (int t = 0; t <= static_cast<int>(n); ++t) {
      const bool one = t < static_cast<int>(n) && host[32 + t] == 1.0f;
      if (one && run_lo < 0) run_lo = t;
      if (!one && run_lo >= 0) {
        if (t - run_lo > best_hi - best_lo) {
          best_lo = run_lo;
          best_hi = t;
        }
        run_lo = -1;
      }
    }
    e.flat_lo = best_lo;
    e.flat_hi = best_hi;
    if (lanes_at) window_lanes::build(host.data() + 32, host.data() + lanes_at);
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&e.dev), host.size() * sizeof(float)));
    HIP_TRY(h, hipMemcpy(e.dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (lanes_at) e.dev_lanes = e.dev + lanes_at;
  }
  h->windows.push_back(e);
  *out = &h->windows.back();
  return FLACENC_HIP_OK;
}

int get_window(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg, uint32_t n, const WindowEntry** out) {
  return get_window_entry(h, cfg->window_type, cfg->tukey_alpha, 0, 0, n, out);
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" {

int flacenc_hip_window_weights(const flacenc_hip_qlpc_config* cfg, uint32_t block_size, float* out) {
  if (!cfg || !out) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  int rc = flacenc_hip_verify_config(cfg);
  if (rc != FLACENC_HIP_OK) return rc;
  window_weights(cfg->window_type, cfg->tukey_alpha, block_size, out);
  return FLACENC_HIP_OK;
}

int flacenc_hip_set_lpc_windows(flacenc_hip_handle* h, const uint32_t* types, const float* alphas,
                                const uint32_t* starts, const uint32_t* ends, uint32_t n_extra) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if (n_extra > FLACENC_HIP_MAX_LPC_WINDOWS - 1 || (n_extra > 0 && (!types || !alphas || !starts || !ends))) {
    h->last_error = "flacenc_hip_set_lpc_windows: at most 7 extra windows, arrays required";
    return FLACENC_HIP_ERR_BAD_CONFIG;
  }
  std::vector<LpcWindow> list;
  for (uint32_t i = 0; i < n_extra; ++i) {
    if (!lpc_window_ok(types[i], alphas[i], starts[i], ends[i])) {
      h->last_error = "flacenc_hip_set_lpc_windows: unknown type, alpha outside [0, 1], or a piece outside 0 <= start < "
                      "end <= 65536";
      return FLACENC_HIP_ERR_BAD_CONFIG;
    }
    list.push_back(LpcWindow{types[i], alphas[i], starts[i], ends[i]});
  }
  h->lpc_windows.swap(list);  // (the weights already cached stay until flacenc_hip_destroy)
  return FLACENC_HIP_OK;
}

int flacenc_hip_lpc_window_weights(uint32_t type, float alpha, uint32_t start, uint32_t end, uint32_t block_size,
                                   float* out) {
  if (!lpc_window_ok(type, alpha, start, end)) return FLACENC_HIP_ERR_BAD_CONFIG;
  if (block_size > FLACENC_HIP_MAX_BLOCK_SIZE || (!out && block_size > 0)) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  lpc_window_weights(type, alpha, start, end, block_size, out);
  return FLACENC_HIP_OK;
}

}  // extern "C"
