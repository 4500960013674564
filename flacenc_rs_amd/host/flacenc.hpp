// flacenc.hpp -- C++ host-side mirror of the flacenc-rs API surface around the GPU path.
//
// The reference is a Rust crate; this image has no Rust toolchain, so the host side above the
// C ABI (include/flacenc_hip.h) is written in C++ with the reference's names, argument meaning
// and error behaviour:
//
//   flacenc::config::{Encoder, StereoCoding, SubFrameCoding, Qlpc, Prc, Fixed, OrderSel, Window}
//                                                        src/config.rs:80-432
//   flacenc::error::{VerifyError, EncodeError}           src/error.rs:178, 458
//   flacenc::source::{Source, FrameBuf, MemSource}       src/source.rs:445, 115, 543
//   flacenc::component::{QuantizedParameters, Residual, Lpc, Constant, Verbatim, SubFrame,
//                        ChannelAssignment, Frame, Stream, StreamInfo}   src/component/datatype.rs
//   flacenc::encode_with_fixed_block_size                src/coding.rs:645 (pub, lib.rs:162)
//   Decode (feature "decode")                            src/component/decode.rs
//
// The controller logic (`encode_subframe` src/coding.rs:384-418, `try_stereo_coding` :469-527) and the frames' bit
// writer run on the GPU (flacenc_hip_encode_stereo_frames / _encode_frames and the packers) for every group of frames,
// the tail block below MIN_BLOCK_SIZE_FOR_PREDICTION and a config without predictors included: every Frame of a
// returned Stream carries its bytes (except one too large for the device bit writer, FLACENC_HIP_ERR_UNSUPPORTED of
// the packers), and Stream::to_bytes() is the reference's stream byte for byte but for the MD5 field.  There is no CPU
// implementation of the path here.
// Not mirrored (out of scope): host-side bit writer, container metadata, a single stream's MD5, serde.
// (The MD5 digests of a BATCH of streams come from the device: md5_spans / decode_streams_md5 at the end of this file.)
// Fixed-LPC candidate (`fixed_lpc`, src/coding.rs:298): part of the on-GPU controller -- fused into one kernel for
// 2 channels, block 4096, lpc_order <= 12 and ApproxEnt.partitions a power of two, candidate batches and the deciding
// kernel behind the same entry points everywhere else.
#ifndef FLACENC_HOST_FLACENC_HPP_
#define FLACENC_HOST_FLACENC_HPP_

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <variant>
#include <vector>

#include "flacenc_hip.h"

namespace flacenc {

// ---------------------------------------------------------------- constant.rs ----
namespace constant {
constexpr size_t DEFAULT_BLOCK_SIZE = 4096;            // src/constant.rs:32
constexpr size_t MIN_BLOCK_SIZE = 32;                  // :45
constexpr size_t MAX_BLOCK_SIZE = 32767;               // :57
constexpr size_t MIN_BLOCK_SIZE_FOR_PREDICTION = 64;   // :51
constexpr size_t MIN_BITS_PER_SAMPLE = 8;              // :38
constexpr size_t MAX_BITS_PER_SAMPLE = 24;             // :54
constexpr size_t MAX_CHANNELS = 8;                     // :60
namespace qlpc {
constexpr size_t DEFAULT_ORDER = 10;       // :109
constexpr size_t DEFAULT_PRECISION = 15;   // :112
constexpr float DEFAULT_TUKEY_ALPHA = 0.4f;  // :115
constexpr size_t MAX_ORDER = 24;           // :118
constexpr size_t MAX_PRECISION = 15;
}  // namespace qlpc
namespace rice {
constexpr size_t MAX_RICE_PARAMETER = 30;  // :143
}
}  // namespace constant

// ------------------------------------------------------------------- error.rs ----
namespace error {
// VerifyError, src/error.rs:178: component path + reason
struct VerifyError : std::runtime_error {
  std::string component;
  VerifyError(std::string comp, const std::string& reason)
      : std::runtime_error("verification error: `" + comp + "` is not valid. reason: " + reason),
        component(std::move(comp)) {}
  VerifyError within(const std::string& outer) const {  // src/error.rs:216
    const std::string what_s = what();
    const size_t pos = what_s.find("reason: ");
    return VerifyError(outer + "." + component, pos == std::string::npos ? what_s : what_s.substr(pos + 8));
  }
};
// EncodeError, src/error.rs:458: Source | Config
struct EncodeError : std::runtime_error {
  enum Kind { Source, Config, Device } kind;
  EncodeError(Kind k, const std::string& msg) : std::runtime_error(msg), kind(k) {}
};
}  // namespace error

// ------------------------------------------------------------------ config.rs ----
namespace config {
struct Window {  // src/config.rs:344-359
  enum Type { Rectangle, Tukey } type = Tukey;
  float alpha = constant::qlpc::DEFAULT_TUKEY_ALPHA;
  void verify() const {  // :371-387
    if (type == Tukey && !(alpha >= 0.0f && alpha <= 1.0f))
      throw error::VerifyError("tukey.alpha", "alpha must be in range between 0 and 1");
  }
};
struct OrderSel {  // :400-409
  enum Type { BitCount, ApproxEnt } type = ApproxEnt;
  size_t partitions = 16;
};
struct Prc {  // :211-214
  size_t max_parameter = constant::rice::MAX_RICE_PARAMETER;
  void verify() const {
    if (max_parameter > constant::rice::MAX_RICE_PARAMETER)
      throw error::VerifyError("max_parameter", "must be in range ..=30");
  }
};
struct Fixed {  // :236-244
  size_t max_order = 4;
  OrderSel order_sel;
  void verify() const {  // :246-255, :419-431
    if (max_order > 4) throw error::VerifyError("max_order", "must be in range ..=4");
    if (order_sel.type == OrderSel::ApproxEnt && (order_sel.partitions < 1 || order_sel.partitions > 64))
      throw error::VerifyError("order_sel.ApproxEnt.partitions", "must be in range 1..=64");
  }
};
struct Qlpc {  // :271-288
  size_t lpc_order = constant::qlpc::DEFAULT_ORDER;
  size_t quant_precision = constant::qlpc::DEFAULT_PRECISION;
  bool use_direct_mse = false;
  size_t mae_optimization_steps = 0;
  Window window;
  void verify() const {  // :302-326
    if (lpc_order < 1 || lpc_order > constant::qlpc::MAX_ORDER)
      throw error::VerifyError("lpc_order", "must be in range 1..=24");
    if (quant_precision < 1 || quant_precision > constant::qlpc::MAX_PRECISION)
      throw error::VerifyError("quant_precision", "must be in range 1..=15");
    // (the reference rejects these two outside its `experimental` cargo feature, :310-320; this mirror follows
    // the experimental build -- the GPU library implements both estimators, include/flacenc_hip.h)
    if (mae_optimization_steps > FLACENC_HIP_MAX_MAE_STEPS)
      throw error::VerifyError("mae_optimization_steps", "must be at most 64 here");
    try {
      window.verify();
    } catch (const error::VerifyError& e) {
      throw e.within("window");
    }
  }
};
struct SubFrameCoding {  // :167-183
  bool use_constant = true;
  bool use_fixed = true;
  bool use_lpc = true;
  Fixed fixed;
  Qlpc qlpc;
  Prc prc;
  void verify() const {  // :198-204
    try {
      fixed.verify();
    } catch (const error::VerifyError& e) {
      throw e.within("fixed");
    }
    try {
      qlpc.verify();
    } catch (const error::VerifyError& e) {
      throw e.within("qlpc");
    }
    try {
      prc.verify();
    } catch (const error::VerifyError& e) {
      throw e.within("prc");
    }
  }
};
struct StereoCoding {  // :137-144
  bool use_leftside = true;
  bool use_rightside = true;
  bool use_midside = true;
};
struct Encoder {  // :85-99
  size_t block_size = constant::DEFAULT_BLOCK_SIZE;
  bool multithread = true;
  StereoCoding stereo_coding;
  SubFrameCoding subframe_coding;
  void verify() const {  // :114-130
    if (block_size < constant::MIN_BLOCK_SIZE || block_size > constant::MAX_BLOCK_SIZE)
      throw error::VerifyError("block_size", "must be in range 32..=32767");
    try {
      subframe_coding.verify();
    } catch (const error::VerifyError& e) {
      throw e.within("subframe_coding");
    }
  }
};
}  // namespace config

// ------------------------------------------------------------------ source.rs ----
namespace source {
// FrameBuf, src/source.rs:115-127: channel-major i32, channel c at [c*size, c*size + filled)
class FrameBuf {
 public:
  FrameBuf(size_t channels, size_t size) : samples_(channels * size, 0), channels_(channels), size_(size) {}
  size_t size() const { return size_; }
  size_t channels() const { return channels_; }
  size_t filled_size() const { return filled_; }
  const int32_t* channel_slice(size_t ch) const { return samples_.data() + ch * size_; }  // :251-253
  int32_t* channel_slice_mut(size_t ch) { return samples_.data() + ch * size_; }
  const int32_t* raw() const { return samples_.data(); }
  // Fill::fill_interleaved, src/source.rs:42-70
  void fill_interleaved(const int32_t* interleaved, size_t n_samples_total) {
    const size_t per_ch = n_samples_total / channels_;
    for (size_t c = 0; c < channels_; ++c) {
      int32_t* dst = channel_slice_mut(c);
      for (size_t t = 0; t < per_ch; ++t) dst[t] = interleaved[t * channels_ + c];
      for (size_t t = per_ch; t < size_; ++t) dst[t] = 0;
    }
    filled_ = per_ch;
  }
  // verify_samples, src/source.rs:262-275
  void verify_samples(size_t bits_per_sample) const {
    const int32_t lo = -(1 << (bits_per_sample - 1)), hi = (1 << (bits_per_sample - 1)) - 1;
    for (size_t c = 0; c < channels_; ++c)
      for (size_t t = 0; t < filled_; ++t) {
        const int32_t v = channel_slice(c)[t];
        if (v < lo || v > hi) throw error::VerifyError("samples", "sample out of range for bits_per_sample");
      }
  }

 private:
  std::vector<int32_t> samples_;
  size_t channels_, size_, filled_ = 0;
};

// Source, src/source.rs:445-480
class Source {
 public:
  virtual ~Source() = default;
  virtual size_t channels() const = 0;
  virtual size_t bits_per_sample() const = 0;
  virtual size_t sample_rate() const = 0;
  // reads up to block_size inter-channel samples into dest; returns the count read (0 = end)
  virtual size_t read_samples(size_t block_size, FrameBuf& dest) = 0;
};

// MemSource, src/source.rs:543-600
class MemSource : public Source {
 public:
  static MemSource from_samples(const std::vector<int32_t>& interleaved, size_t channels,
                                size_t bits_per_sample, size_t sample_rate) {
    MemSource s;
    s.samples_ = interleaved;
    s.channels_ = channels;
    s.bps_ = bits_per_sample;
    s.rate_ = sample_rate;
    return s;
  }
  size_t channels() const override { return channels_; }
  size_t bits_per_sample() const override { return bps_; }
  size_t sample_rate() const override { return rate_; }
  size_t read_samples(size_t block_size, FrameBuf& dest) override {
    const size_t begin = pos_ * channels_;
    const size_t end = std::min(samples_.size(), begin + block_size * channels_);
    if (end <= begin) return 0;
    dest.fill_interleaved(samples_.data() + begin, end - begin);
    const size_t n = (end - begin) / channels_;
    pos_ += n;
    return n;
  }
  size_t len_hint() const { return samples_.size() / channels_; }

 private:
  std::vector<int32_t> samples_;
  size_t channels_ = 1, bps_ = 16, rate_ = 44100, pos_ = 0;
};
}  // namespace source

// ------------------------------------------------------------------ component ----
namespace component {
// rice::encode_signbit / decode_signbit, src/rice.rs:169-187
inline uint32_t encode_signbit(int32_t v) { return (static_cast<uint32_t>(v) << 1) ^ static_cast<uint32_t>(v >> 31); }
inline int32_t decode_signbit(uint32_t v) { return static_cast<int32_t>(v >> 1) ^ -static_cast<int32_t>(v & 1u); }

// QuantizedParameters, src/component/datatype.rs:2164-2170
struct QuantizedParameters {
  int16_t coefs[32] = {0};
  size_t order = 0;
  int8_t shift = 0;
  size_t precision = 0;
};

// Residual, src/component/datatype.rs:2269-2284 (quotients/remainders derived on demand,
// src/coding.rs:58-62, 140-170)
struct Residual {
  uint8_t partition_order = 0;
  size_t block_size = 0;
  size_t warmup_length = 0;
  std::vector<uint8_t> rice_params;
  std::vector<int32_t> errors;  // first warmup_length slots are zero
  uint64_t sum_quotients = 0;
  uint64_t sum_rice_params = 0;
  std::pair<uint32_t, uint32_t> quotient_and_remainder(size_t t) const {
    if (t < warmup_length) return {0u, 0u};
    const uint8_t p = rice_params[t / (block_size >> partition_order)];
    const uint32_t u = encode_signbit(errors[t]);
    return {u >> p, u & ((1u << p) - 1u)};
  }
  // BitRepr::count_bits, src/component/bitrepr.rs:533-544
  size_t count_bits() const {
    const size_t nparts = size_t(1) << partition_order;
    bool rice2 = false;
    for (size_t i = 0; i < nparts; ++i) rice2 |= rice_params[i] > 14;
    return 2 + 4 + nparts * (rice2 ? 5 : 4) + (sum_quotients + block_size - warmup_length) +
           (sum_rice_params * (block_size >> partition_order) - warmup_length * rice_params[0]);
  }
  // Decode::copy_signal, src/component/decode.rs:226-237
  void copy_signal(int32_t* dest) const {
    for (size_t t = 0; t < block_size; ++t) {
      auto qr = quotient_and_remainder(t);
      const uint8_t p = rice_params[t / (block_size >> partition_order)];
      dest[t] = decode_signbit((qr.first << p) + qr.second);
    }
  }
};

struct Constant {  // datatype.rs:1820
  size_t block_size;
  int32_t dc_offset;
  uint8_t bits_per_sample;
  size_t count_bits() const { return 8 + bits_per_sample; }  // bitrepr.rs:445
};
struct Verbatim {  // datatype.rs:1896
  std::vector<int32_t> samples;
  uint8_t bits_per_sample;
  static size_t count_bits_from_metadata(size_t n, size_t bps) { return 8 + n * bps; }  // datatype.rs:1944
  size_t count_bits() const { return count_bits_from_metadata(samples.size(), bits_per_sample); }
};
struct Lpc {  // datatype.rs:2057-2062
  QuantizedParameters parameters;
  std::vector<int32_t> warm_up;
  Residual residual;
  uint8_t bits_per_sample;
  size_t order() const { return parameters.order; }
  size_t count_bits() const {  // bitrepr.rs:492-499
    return 8 + size_t(bits_per_sample) * order() + 4 + 5 + parameters.precision * order() + residual.count_bits();
  }
};
struct FixedLpc {  // datatype.rs:1960-1964
  std::vector<int32_t> warm_up;
  Residual residual;
  uint8_t bits_per_sample;
  size_t order() const { return warm_up.size(); }
  size_t count_bits() const {  // bitrepr.rs:473-477
    return 8 + size_t(bits_per_sample) * order() + residual.count_bits();
  }
};
using SubFrame = std::variant<Constant, Verbatim, FixedLpc, Lpc>;  // datatype.rs:1782
inline size_t count_bits(const SubFrame& sf) {
  return std::visit([](const auto& c) { return c.count_bits(); }, sf);
}

// Decode for SubFrame, src/component/decode.rs:116-218
inline std::vector<int32_t> decode(const SubFrame& sf) {
  if (const auto* c = std::get_if<Constant>(&sf)) return std::vector<int32_t>(c->block_size, c->dc_offset);
  if (const auto* v = std::get_if<Verbatim>(&sf)) return v->samples;
  if (const auto* fx = std::get_if<FixedLpc>(&sf)) {  // decode.rs:179-201
    static const int32_t kFixedCoefs[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
    std::vector<int32_t> dest(fx->residual.block_size);
    fx->residual.copy_signal(dest.data());
    const size_t order = fx->order();
    for (size_t t = 0; t < order; ++t) dest[t] = fx->warm_up[t];
    for (size_t t = order; t < dest.size(); ++t) {
      int64_t pred = 0;
      for (size_t tau = 0; tau < order; ++tau) pred += int64_t(kFixedCoefs[order][tau]) * int64_t(dest[t - 1 - tau]);
      dest[t] = int32_t(uint32_t(dest[t]) + uint32_t(int32_t(pred)));
    }
    return dest;
  }
  const Lpc& l = std::get<Lpc>(sf);
  std::vector<int32_t> dest(l.residual.block_size);
  l.residual.copy_signal(dest.data());
  for (size_t t = 0; t < l.warm_up.size(); ++t) dest[t] = l.warm_up[t];
  for (size_t t = l.warm_up.size(); t < dest.size(); ++t) {  // decode_lpc, decode.rs:159-177
    int64_t pred = 0;
    for (size_t tau = 0; tau < l.order(); ++tau) pred += int64_t(l.parameters.coefs[tau]) * int64_t(dest[t - 1 - tau]);
    dest[t] = int32_t(uint32_t(dest[t]) + uint32_t(int32_t(pred >> l.parameters.shift)));
  }
  return dest;
}

enum class ChannelAssignment { Independent, LeftSide, RightSide, MidSide };  // datatype.rs:1083

struct Frame {  // datatype.rs:820
  uint32_t frame_number = 0;
  size_t block_size = 0;
  ChannelAssignment channel_assignment = ChannelAssignment::Independent;
  std::vector<SubFrame> subframes;
  // Frame::precomputed_bitstream (datatype.rs:820-830): the frame as it goes into the stream;
  // filled by the GPU bit writer (flacenc_hip_pack_stereo_frames) where that path is taken
  std::vector<uint8_t> precomputed_bitstream;
  size_t count_subframe_bits() const {
    size_t b = 0;
    for (const auto& s : subframes) b += count_bits(s);
    return b;
  }
  // Decode for Frame, src/component/decode.rs:61-113: returns channel-major samples
  std::vector<std::vector<int32_t>> decode_channels() const {
    std::vector<std::vector<int32_t>> ch;
    for (const auto& s : subframes) ch.push_back(decode(s));
    if (channel_assignment == ChannelAssignment::LeftSide) {
      for (size_t t = 0; t < block_size; ++t) ch[1][t] = ch[0][t] - ch[1][t];
    } else if (channel_assignment == ChannelAssignment::RightSide) {
      for (size_t t = 0; t < block_size; ++t) ch[0][t] += ch[1][t];
    } else if (channel_assignment == ChannelAssignment::MidSide) {
      for (size_t t = 0; t < block_size; ++t) {
        const int32_t s = ch[1][t];
        const int32_t m = int32_t(uint32_t(ch[0][t]) << 1) + (s & 1);
        ch[0][t] = (m + s) >> 1;
        ch[1][t] = (m - s) >> 1;
      }
    }
    return ch;
  }
};

struct StreamInfo {  // datatype.rs:435-445, defaults :476-479
  size_t sample_rate = 0, channels = 0, bits_per_sample = 0;
  size_t min_block_size = 0xFFFF, max_block_size = 0;
  size_t min_frame_size = 0xFFFFFFFFu, max_frame_size = 0;
  uint64_t total_samples = 0;
  // all zero = "not computed": one stream's MD5 is host work outside this mirror; a host that encodes many files gets
  // all their digests in one call from md5_spans (below)
  uint8_t md5_digest[16] = {0};
  // update_frame_info, datatype.rs:514-523 (total_samples is counted by the encoder loop here)
  void update_frame_info(const Frame& f) {
    min_block_size = std::min(min_block_size, f.block_size);
    max_block_size = std::max(max_block_size, f.block_size);
    if (!f.precomputed_bitstream.empty()) {
      min_frame_size = std::min(min_frame_size, f.precomputed_bitstream.size());
      max_frame_size = std::max(max_frame_size, f.precomputed_bitstream.size());
    }
  }
};
struct Stream {  // datatype.rs:65
  StreamInfo stream_info;
  std::vector<Frame> frames;
  void add_frame(Frame f) {  // datatype.rs:184-187
    stream_info.update_frame_info(f);
    frames.push_back(std::move(f));
  }
  // BitRepr for Stream::write (bitrepr.rs:185-196): "fLaC", the STREAMINFO block (:207-216,
  // :246-270, last-block flag set as Stream::write does for a stream without further metadata),
  // then every frame's precomputed bitstream (:290-293).  A frame that the GPU bit writer refused as too large
  // has none: the host-side bit writer is outside this mirror.
  std::vector<uint8_t> to_bytes() const {
    std::vector<uint8_t> out = {0x66, 0x4c, 0x61, 0x43, 0x80, 0x00, 0x00, 34};
    auto be = [&](uint64_t v, int bytes) {
      for (int i = bytes - 1; i >= 0; --i) out.push_back(uint8_t(v >> (8 * i)));
    };
    be(stream_info.min_block_size, 2);
    be(stream_info.max_block_size, 2);
    be(stream_info.min_frame_size & 0xFFFFFF, 3);
    be(stream_info.max_frame_size & 0xFFFFFF, 3);
    be((uint64_t(stream_info.sample_rate) << 44) | (uint64_t(stream_info.channels - 1) << 41) |
           (uint64_t(stream_info.bits_per_sample - 1) << 36) | (stream_info.total_samples & 0xFFFFFFFFFull),
       8);
    out.insert(out.end(), stream_info.md5_digest, stream_info.md5_digest + 16);
    for (const Frame& f : frames) {
      if (f.precomputed_bitstream.empty())
        throw std::runtime_error("Stream::to_bytes: a frame has no precomputed bitstream (too large for "
                                 "the GPU bit writer)");
      out.insert(out.end(), f.precomputed_bitstream.begin(), f.precomputed_bitstream.end());
    }
    return out;
  }
};
}  // namespace component

// ----------------------------------------------------------------- the GPU side ----
// RAII owner of a flacenc_hip_handle (the role of the reference's per-thread scratch)
// What HipContext::encode_variable gives back: the chosen frames back to back, per frame its offset, length and block
// size, per superblock its split mask (bit n - 1: heap node n split; include/flacenc_hip.h).
struct VariableFrames {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lengths, block_sizes, split_masks;
};

class HipContext {
 public:
  explicit HipContext(int device_id = 0) {
    // (flacenc_hip_qlpc_config is embedded by value in the frame config: a library of another ABI revision would read
    // every field behind it shifted)
    if (flacenc_hip_abi_version() != FLACENC_HIP_ABI_VERSION)
      throw error::EncodeError(error::EncodeError::Device, "libflacenc_hip.so has another ABI revision than include/flacenc_hip.h");
    const int rc = flacenc_hip_create(&h_, device_id);
    if (rc != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, "flacenc_hip_create failed (no usable GPU)");
  }
  ~HipContext() {
    if (h_) flacenc_hip_destroy(h_);
  }
  HipContext(const HipContext&) = delete;
  HipContext& operator=(const HipContext&) = delete;
  HipContext(HipContext&& o) noexcept  // std::vector<HipContext>: one per GPU
      : h_(o.h_), sum_order_(o.sum_order_), order_search_(o.order_search_), window_search_(o.window_search_),
        order_guess_(o.order_guess_), precision_search_(o.precision_search_) {
    o.h_ = nullptr;
  }
  HipContext& operator=(HipContext&& o) noexcept {
    if (this != &o) {
      if (h_) flacenc_hip_destroy(h_);
      h_ = o.h_;
      sum_order_ = o.sum_order_;
      order_search_ = o.order_search_;
      window_search_ = o.window_search_;
      order_guess_ = o.order_guess_;
      precision_search_ = o.precision_search_;
      o.h_ = nullptr;
    }
    return *this;
  }
  flacenc_hip_handle* get() const { return h_; }

  // Which build of the crate the floating-point sums of the path reproduce bit for bit: the stable build
  // (one mul_add chain per lag, src/lpc.rs:533-548; one f32 chain per estimator partition,
  // src/arrayutils.rs:435-506), the `simd-nightly` build (src/lpc.rs:439-531; LPC orders up to 15 -- above,
  // the unflagged order is used), or the library's unflagged mode (Canonical: since ABI 6 the stable build's quantised LPC
  // parameters on every shape -- certified on blocks of 4096 / 4608, the stable build's own chains elsewhere -- with the
  // fixed-LPC selector's sums exact integers rather than that build's f32 chains, which only matters above 16 bits).
  enum class SumOrder { Canonical, Stable, SimdNightly };
  // Wasted bits k of output channel c of a record (FLACENC_HIP_FLAG_WASTED_BITS; 0 without it)
  static uint32_t wasted_bits(const flacenc_hip_stereo_frame_result& r, int c) { return r.pad[c]; }
  static uint32_t wasted_bits(const flacenc_hip_channel_result& r) { return r.pad[0]; }
  void set_sum_order(SumOrder o) { sum_order_ = o; }
  SumOrder sum_order() const { return sum_order_; }
  // (never FLACENC_HIP_FLAG_WASTED_BITS: the SubFrame rebuilt from the records has no wasted-bits field; a caller of
  // encode_variable may pass it in cfg, and the frames' bytes then carry the wasted bits.  Nor
  // FLACENC_HIP_FLAG_RICE_ESCAPE: component::Residual holds Rice parameters only, and a record with a partition marked
  // 0x80 | width has no SubFrame; encode_variable takes the flag in cfg in the same way)
  // FLACENC_HIP_FLAG_ORDER_SEARCH: every LPC subframe's order searched over 1..lpc_order (the records stay ordinary
  // SubFrame::Lpc of the chosen order); off by default
  void set_order_search(bool on) { order_search_ = on; }
  bool order_search() const { return order_search_; }
  // FLACENC_HIP_FLAG_WINDOW_SEARCH: every LPC subframe analysed under the config's window and the handle's extra windows
  // (set_lpc_windows; a fresh handle holds the header's default list), the shortest kept; off by default
  void set_window_search(bool on) { window_search_ = on; }
  bool window_search() const { return window_search_; }
  // the extra windows, (type, alpha, start, end) entry by entry (flacenc_hip_set_lpc_windows; n_extra <= 7)
  void set_lpc_windows(const uint32_t* types, const float* alphas, const uint32_t* starts, const uint32_t* ends,
                       uint32_t n_extra) {
    if (flacenc_hip_set_lpc_windows(h_, types, alphas, starts, ends, n_extra) != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
  }
  // FLACENC_HIP_FLAG_ORDER_GUESS: every LPC subframe's order guessed from the Levinson error and only (0, lpc_order) and
  // the guesses coded (set_order_guesses: how many per window, 1 on a fresh handle); off by default, and not to be
  // combined with set_order_search (the library answers FLACENC_HIP_ERR_BAD_CONFIG)
  void set_order_guess(bool on) { order_guess_ = on; }
  bool order_guess() const { return order_guess_; }
  void set_order_guesses(uint32_t k) {
    if (flacenc_hip_set_order_guesses(h_, k) != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
  }
  // FLACENC_HIP_FLAG_PRECISION_SEARCH: every LPC subframe coded at each coefficient precision from quant_precision down to
  // the handle's floor (set_precision_floor: kDefaultPrecisionFloor on a fresh handle), the shortest kept (the records
  // stay ordinary SubFrame::Lpc at the chosen precision); off by default
  static constexpr uint32_t kDefaultPrecisionFloor = 5;
  void set_precision_search(bool on) { precision_search_ = on; }
  bool precision_search() const { return precision_search_; }
  void set_precision_floor(uint32_t floor) {
    if (flacenc_hip_set_precision_floor(h_, floor) != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
  }
  // the deepest FLAC stream the handle's decode calls take: 24 (a fresh handle, the reference's limit) or 32
  // (flacenc_hip_set_max_bits_per_sample); the encode calls do not read it
  void set_max_bits_per_sample(uint32_t bits) {
    if (flacenc_hip_set_max_bits_per_sample(h_, bits) != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
  }
  // the deepest PCM the handle's stream-level encode calls take: 24 (a fresh handle) or 32
  // (flacenc_hip_set_max_encode_bits_per_sample); more than 24 bits come in 4-byte samples and run the wide path
  void set_max_encode_bits_per_sample(uint32_t bits) {
    if (flacenc_hip_set_max_encode_bits_per_sample(h_, bits) != FLACENC_HIP_OK)
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
  }
  uint32_t sum_order_flags(size_t lpc_order) const {
    const uint32_t os = (order_search_ ? FLACENC_HIP_FLAG_ORDER_SEARCH : 0u) | (window_search_ ? FLACENC_HIP_FLAG_WINDOW_SEARCH : 0u) |
                        (order_guess_ ? FLACENC_HIP_FLAG_ORDER_GUESS : 0u) |
                        (precision_search_ ? FLACENC_HIP_FLAG_PRECISION_SEARCH : 0u);
    // (the mirror consumes integers only: certified shapes keep their own order, INTEGER_PARITY_ONLY)
    if (sum_order_ == SumOrder::Stable) return FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER | FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY | os;
    if (sum_order_ == SumOrder::SimdNightly && lpc_order <= 15) return FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER | os;
    return os;
  }

  // The block-size search (flacenc_hip_encode_variable, host memory): `frames` in FrameBuf layout, channel c of
  // superblock i at frames + (i * channels + c) * block_size, zero beyond total_samples.
  VariableFrames encode_variable(const flacenc_hip_frame_config& cfg, const int32_t* frames, uint64_t total_samples,
                                 uint32_t channels, uint32_t block_size, uint32_t levels, uint32_t bits_per_sample,
                                 uint32_t sample_rate, uint64_t first_sample_number = 0) {
    const size_t cap = flacenc_hip_variable_bytes_bound(channels, block_size, levels, bits_per_sample, total_samples);
    const size_t max_frames = flacenc_hip_variable_max_frames(block_size, levels, total_samples);
    if (cap == 0 && total_samples != 0)
      throw error::EncodeError(error::EncodeError::Device, "encode_variable: channels, block size or levels rejected");
    VariableFrames v;
    v.bytes.resize(cap);
    v.offsets.resize(max_frames);
    v.lengths.resize(max_frames);
    v.block_sizes.resize(max_frames);
    v.split_masks.resize((total_samples + block_size - 1) / block_size);
    uint64_t totals[2] = {0, 0};
    const int rc = flacenc_hip_encode_variable(h_, &cfg, frames, total_samples, channels, block_size, levels, block_size,
                                               bits_per_sample, sample_rate, first_sample_number, v.bytes.data(), cap,
                                               v.offsets.data(), v.lengths.data(), v.block_sizes.data(), max_frames,
                                               v.split_masks.data(), totals, FLACENC_HIP_MEM_HOST);
    if (rc != FLACENC_HIP_OK || (totals[0] & FLACENC_HIP_VARIABLE_OVERFLOW))
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(h_));
    v.bytes.resize(totals[1]);
    v.offsets.resize(totals[0]);
    v.lengths.resize(totals[0]);
    v.block_sizes.resize(totals[0]);
    return v;
  }

 private:
  flacenc_hip_handle* h_ = nullptr;
  SumOrder sum_order_ = SumOrder::Canonical;
  bool order_search_ = false;
  bool window_search_ = false;
  bool order_guess_ = false;
  bool precision_search_ = false;
};

// Staging memory for the host-pointer entry points: page-locked (flacenc_hip_host_alloc), so that the
// library's copies are plain DMA transfers instead of going through the driver's bounce buffers -- the
// role of the reference's reused FrameBuf pool (src/par.rs:364-368).  Falls back to ordinary memory if
// page-locked memory cannot be had.
template <class T>
class PinnedBuffer {
 public:
  explicit PinnedBuffer(size_t count) : count_(count) {
    if (count == 0) return;
    ptr_ = static_cast<T*>(flacenc_hip_host_alloc(count * sizeof(T)));
    if (ptr_ == nullptr) {
      fallback_.resize(count);
      ptr_ = fallback_.data();
    }
  }
  ~PinnedBuffer() {
    if (ptr_ != nullptr && fallback_.empty()) flacenc_hip_host_free(ptr_);
  }
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  T* data() { return ptr_; }
  const T* data() const { return ptr_; }
  T& operator[](size_t i) { return ptr_[i]; }
  const T& operator[](size_t i) const { return ptr_[i]; }
  T* begin() { return ptr_; }
  size_t size() const { return count_; }

 private:
  T* ptr_ = nullptr;
  size_t count_ = 0;
  std::vector<T> fallback_;
};

namespace detail {
inline flacenc_hip_qlpc_config to_abi(const config::SubFrameCoding& c) {
  flacenc_hip_qlpc_config o{};
  o.lpc_order = static_cast<uint32_t>(c.qlpc.lpc_order);
  o.quant_precision = static_cast<uint32_t>(c.qlpc.quant_precision);
  o.window_type = c.qlpc.window.type == config::Window::Rectangle ? FLACENC_HIP_WINDOW_RECTANGLE
                                                                  : FLACENC_HIP_WINDOW_TUKEY;
  o.tukey_alpha = c.qlpc.window.alpha;
  o.max_rice_parameter = static_cast<uint32_t>(c.prc.max_parameter);
  o.flags = 0;
  o.use_direct_mse = c.qlpc.use_direct_mse ? 1u : 0u;
  o.mae_optimization_steps = static_cast<uint32_t>(c.qlpc.mae_optimization_steps);
  return o;
}

// SubFrame::Lpc from one GPU record + residual row (Lpc::from_parts, coding.rs:373-380)
inline component::Lpc make_lpc(const flacenc_hip_subframe_params& p, const int32_t* residual,
                               const int32_t* signal, size_t n, uint8_t bps) {
  component::Lpc l;
  std::memcpy(l.parameters.coefs, p.coefs, sizeof(p.coefs));
  l.parameters.order = p.order;
  l.parameters.shift = p.shift;
  l.parameters.precision = p.precision;
  l.warm_up.assign(signal, signal + p.order);
  l.residual.partition_order = p.rice_order;
  l.residual.block_size = n;
  l.residual.warmup_length = p.order;
  l.residual.rice_params.assign(p.rice_params, p.rice_params + (size_t(1) << p.rice_order));
  l.residual.errors.assign(residual, residual + n);
  l.residual.sum_quotients = p.sum_quotients;
  l.residual.sum_rice_params = 0;
  for (uint8_t v : l.residual.rice_params) l.residual.sum_rice_params += v;
  l.bits_per_sample = bps;
  return l;
}

// SubFrame::FixedLpc from one GPU record + error-signal row (FixedLpc::from_parts, coding.rs:321-328)
inline component::FixedLpc make_fixed_lpc(const flacenc_hip_subframe_params& p, const int32_t* residual,
                                          const int32_t* signal, size_t n, uint8_t bps) {
  component::FixedLpc fx;
  fx.warm_up.assign(signal, signal + p.order);
  fx.residual.partition_order = p.rice_order;
  fx.residual.block_size = n;
  fx.residual.warmup_length = p.order;
  fx.residual.rice_params.assign(p.rice_params, p.rice_params + (size_t(1) << p.rice_order));
  fx.residual.errors.assign(residual, residual + n);
  fx.residual.sum_quotients = p.sum_quotients;
  fx.residual.sum_rice_params = 0;
  for (uint8_t v : fx.residual.rice_params) fx.residual.sum_rice_params += v;
  fx.bits_per_sample = bps;
  return fx;
}
}  // namespace detail

namespace detail {
// encode_fixed_size_frame (src/coding.rs:581-606) for a run of frames on ONE GPU: `bufs[i]` is stream
// frame first_number + i*number_step (number_step > 1 when frames were dealt round-robin over several
// GPUs).  Frames of equal filled size (all but the stream's last) are coded in one batch; the reference's
// per-frame controller (encode_frame, coding.rs:530-544) and its bit writer run on the device for every group.
inline std::vector<component::Frame> encode_frame_run(const config::Encoder& config,
                                                      const std::vector<const source::FrameBuf*>& bufs,
                                                      size_t first_number, size_t number_step, size_t nch,
                                                      size_t bps, size_t sample_rate, HipContext& gpu) {
  const config::SubFrameCoding& sc = config.subframe_coding;
  std::vector<component::Frame> out;
  out.reserve(bufs.size());
  flacenc_hip_qlpc_config abi_cfg = detail::to_abi(sc);
  abi_cfg.flags |= gpu.sum_order_flags(sc.qlpc.lpc_order);
  const bool stereo = (nch == 2);

  // 2. group frames by filled size (all but the last are block_size) and batch each group
  size_t f0 = 0;
  while (f0 < bufs.size()) {
    const size_t n = bufs[f0]->filled_size();
    size_t f1 = f0;
    while (f1 < bufs.size() && bufs[f1]->filled_size() == n) ++f1;
    const size_t nf = f1 - f0;
    // 2a. stereo: encode_frame on the GPU (flacenc_hip_encode_stereo_frames), its records turned into Frames directly,
    //     and the frames' bytes (flacenc_hip_pack_stereo_frames).  A block below MIN_BLOCK_SIZE_FOR_PREDICTION and a
    //     config with neither predictor go the same way: the library codes them Constant / Verbatim (too_short,
    //     coding.rs:396).
    if (stereo) {
      PinnedBuffer<int32_t> staged(nf * 2 * n);
      for (size_t f = 0; f < nf; ++f)
        for (size_t c = 0; c < 2; ++c)
          std::memcpy(&staged[(f * 2 + c) * n], bufs[f0 + f]->channel_slice(c), n * sizeof(int32_t));
      flacenc_hip_frame_config fc{};
      fc.qlpc = abi_cfg;
      fc.use_constant = sc.use_constant;
      fc.use_fixed = sc.use_fixed;
      fc.fixed_max_order = static_cast<uint32_t>(sc.fixed.max_order);
      fc.fixed_order_sel = sc.fixed.order_sel.type == config::OrderSel::BitCount ? FLACENC_HIP_ORDERSEL_BITCOUNT
                                                                                 : FLACENC_HIP_ORDERSEL_APPROXENT;
      fc.fixed_partitions = static_cast<uint32_t>(sc.fixed.order_sel.partitions);
      fc.use_lpc = sc.use_lpc;
      fc.use_leftside = config.stereo_coding.use_leftside;
      fc.use_rightside = config.stereo_coding.use_rightside;
      fc.use_midside = config.stereo_coding.use_midside;
      std::vector<flacenc_hip_stereo_frame_result> fr(nf);
      PinnedBuffer<int32_t> resid2(nf * 2 * n);
      const int rc = flacenc_hip_encode_stereo_frames(gpu.get(), &fc, staged.data(), nf, static_cast<uint32_t>(n), n,
                                                      static_cast<uint32_t>(bps), fr.data(), resid2.data(), n,
                                                      FLACENC_HIP_MEM_HOST);
      if (rc == FLACENC_HIP_OK) {
        // Frame::write on the GPU too (bitrepr.rs:289-319): the frames' final bytes
        const size_t ostride = flacenc_hip_stereo_frame_bytes_bound(static_cast<uint32_t>(n), static_cast<uint32_t>(bps));
        PinnedBuffer<uint8_t> packed(nf * ostride);
        std::vector<uint32_t> packed_len(nf);
        const int prc = flacenc_hip_pack_stereo_frames(
            gpu.get(), staged.data(), nf, static_cast<uint32_t>(n), n, fr.data(), resid2.data(), n,
            static_cast<uint32_t>(bps), static_cast<uint32_t>(sample_rate), static_cast<uint32_t>(first_number + f0 * number_step),
            static_cast<uint32_t>(number_step),
            packed.data(), ostride, packed_len.data(), FLACENC_HIP_MEM_HOST);
        if (prc != FLACENC_HIP_OK && prc != FLACENC_HIP_ERR_UNSUPPORTED)
          throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
        for (size_t f = 0; f < nf; ++f) {
          // the reference panics where an analysis saw a non-finite or negative-energy autocorrelation
          // (lpc.rs:646, :786-799); the GPU reports it per frame instead
          if (fr[f].analysis_status != FLACENC_HIP_SUBFRAME_OK)
            throw std::runtime_error("LPC analysis reported a non-finite result (lpc.rs:786)");
          const source::FrameBuf& fb = *bufs[f0 + f];
          const int32_t* l = fb.channel_slice(0);
          const int32_t* r = fb.channel_slice(1);
          component::Frame frame;
          frame.frame_number = static_cast<uint32_t>(first_number + (f0 + f) * number_step);
          frame.block_size = n;
          frame.channel_assignment = static_cast<component::ChannelAssignment>(fr[f].channel_assignment);
          for (int c = 0; c < 2; ++c) {
            const int role = fr[f].role[c];
            std::vector<int32_t> sig(n);
            for (size_t t = 0; t < n; ++t)
              sig[t] = role == 0 ? l[t] : role == 1 ? r[t] : role == 2 ? ((l[t] + r[t]) >> 1) : (l[t] - r[t]);
            const uint8_t b = static_cast<uint8_t>(bps + (role == 3 ? 1 : 0));
            if (fr[f].kind[c] == FLACENC_HIP_KIND_CONSTANT) {
              frame.subframes.push_back(component::Constant{n, fr[f].dc_offset[c], b});
            } else if (fr[f].kind[c] == FLACENC_HIP_KIND_VERBATIM) {
              frame.subframes.push_back(component::Verbatim{std::move(sig), b});
            } else if (fr[f].kind[c] == FLACENC_HIP_KIND_FIXED) {
              frame.subframes.push_back(
                  detail::make_fixed_lpc(fr[f].lpc[c], &resid2[(f * 2 + c) * n], sig.data(), n, b));
            } else {
              if (fr[f].lpc[c].status != FLACENC_HIP_SUBFRAME_OK)
                throw std::runtime_error("LPC analysis reported a non-finite result (lpc.rs:786)");
              frame.subframes.push_back(detail::make_lpc(fr[f].lpc[c], &resid2[(f * 2 + c) * n], sig.data(), n, b));
            }
          }
          if (prc == FLACENC_HIP_OK)
            frame.precomputed_bitstream.assign(packed.begin() + f * ostride, packed.begin() + f * ostride + packed_len[f]);
          out.push_back(std::move(frame));
        }
        f0 = f1;
        continue;
      }
      if (rc == FLACENC_HIP_ERR_BAD_CONFIG)
        throw error::EncodeError(error::EncodeError::Config, flacenc_hip_last_error(gpu.get()));
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
    }
    // 2a'. mono / multi-channel: encode_frame for Independent(n) on the GPU (flacenc_hip_encode_frames)
    //      and the frames' bytes (flacenc_hip_pack_frames)
    {
      PinnedBuffer<int32_t> staged(nf * nch * n);
      for (size_t f = 0; f < nf; ++f)
        for (size_t c = 0; c < nch; ++c)
          std::memcpy(&staged[(f * nch + c) * n], bufs[f0 + f]->channel_slice(c), n * sizeof(int32_t));
      flacenc_hip_frame_config fc{};
      fc.qlpc = abi_cfg;
      fc.use_constant = sc.use_constant;
      fc.use_fixed = sc.use_fixed;
      fc.use_lpc = sc.use_lpc;
      fc.fixed_max_order = static_cast<uint32_t>(sc.fixed.max_order);
      fc.fixed_order_sel = sc.fixed.order_sel.type == config::OrderSel::BitCount ? FLACENC_HIP_ORDERSEL_BITCOUNT
                                                                                 : FLACENC_HIP_ORDERSEL_APPROXENT;
      fc.fixed_partitions = static_cast<uint32_t>(sc.fixed.order_sel.partitions);
      std::vector<flacenc_hip_channel_result> cr(nf * nch);
      PinnedBuffer<int32_t> resid2(nf * nch * n);
      const int rc = flacenc_hip_encode_frames(gpu.get(), &fc, staged.data(), nf, static_cast<uint32_t>(nch),
                                               static_cast<uint32_t>(n), n, static_cast<uint32_t>(bps), cr.data(),
                                               resid2.data(), n, FLACENC_HIP_MEM_HOST);
      if (rc == FLACENC_HIP_OK) {
        const size_t ostride = flacenc_hip_frame_bytes_bound(static_cast<uint32_t>(nch), static_cast<uint32_t>(n),
                                                             static_cast<uint32_t>(bps));
        PinnedBuffer<uint8_t> packed(nf * ostride);
        std::vector<uint32_t> packed_len(nf);
        const int prc = flacenc_hip_pack_frames(gpu.get(), staged.data(), nf, static_cast<uint32_t>(nch),
                                                static_cast<uint32_t>(n), n, cr.data(), resid2.data(), n,
                                                static_cast<uint32_t>(bps), static_cast<uint32_t>(sample_rate),
                                                static_cast<uint32_t>(first_number + f0 * number_step),
            static_cast<uint32_t>(number_step), packed.data(), ostride,
                                                packed_len.data(), FLACENC_HIP_MEM_HOST);
        if (prc != FLACENC_HIP_OK && prc != FLACENC_HIP_ERR_UNSUPPORTED)
          throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
        for (size_t f = 0; f < nf; ++f) {
          component::Frame frame;
          frame.frame_number = static_cast<uint32_t>(first_number + (f0 + f) * number_step);
          frame.block_size = n;
          for (size_t c = 0; c < nch; ++c) {
            const flacenc_hip_channel_result& r = cr[f * nch + c];
            if (r.analysis_status != FLACENC_HIP_SUBFRAME_OK)
              throw std::runtime_error("LPC analysis reported a non-finite result (lpc.rs:786)");
            const int32_t* sig = bufs[f0 + f]->channel_slice(c);
            const uint8_t b = static_cast<uint8_t>(bps);
            if (r.kind == FLACENC_HIP_KIND_CONSTANT) {
              frame.subframes.push_back(component::Constant{n, r.dc_offset, b});
            } else if (r.kind == FLACENC_HIP_KIND_VERBATIM) {
              frame.subframes.push_back(component::Verbatim{std::vector<int32_t>(sig, sig + n), b});
            } else if (r.kind == FLACENC_HIP_KIND_FIXED) {
              frame.subframes.push_back(detail::make_fixed_lpc(r.params, &resid2[(f * nch + c) * n], sig, n, b));
            } else {
              if (r.params.status != FLACENC_HIP_SUBFRAME_OK)
                throw std::runtime_error("LPC analysis reported a non-finite result (lpc.rs:786)");
              frame.subframes.push_back(detail::make_lpc(r.params, &resid2[(f * nch + c) * n], sig, n, b));
            }
          }
          if (prc == FLACENC_HIP_OK)
            frame.precomputed_bitstream.assign(packed.begin() + f * ostride, packed.begin() + f * ostride + packed_len[f]);
          out.push_back(std::move(frame));
        }
        f0 = f1;
        continue;
      }
      if (rc == FLACENC_HIP_ERR_BAD_CONFIG)
        throw error::EncodeError(error::EncodeError::Config, flacenc_hip_last_error(gpu.get()));
      throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
    }
  }
  return out;
}

// src/coding.rs:662-674 (serial) / the feed loop of src/par.rs:288-325
template <class SourceT>
std::vector<source::FrameBuf> drain_source(SourceT& src, size_t block_size, size_t nch, size_t bps,
                                           component::Stream& stream) {
  std::vector<source::FrameBuf> bufs;
  for (;;) {
    source::FrameBuf fb(nch, block_size);
    const size_t got = src.read_samples(block_size, fb);
    if (got == 0) break;
    try {  // encode_fixed_size_frame's `verify_samples(..)?` (coding.rs:593): From<VerifyError> for EncodeError is Config
      fb.verify_samples(bps);  // (error.rs:489-491)
    } catch (const error::VerifyError& e) {
      throw error::EncodeError(error::EncodeError::Config, e.what());
    }
    stream.stream_info.total_samples += got;
    bufs.push_back(std::move(fb));
  }
  return bufs;
}

// fixed-block mode exposes one block size in STREAMINFO, the largest block seen (a stream shorter than one block: its
// only frame's); a stream without frames keeps StreamInfo::new's values (coding.rs:676-687)
inline void finalize_block_sizes(component::Stream& stream) {
  if (stream.frames.empty()) return;
  stream.stream_info.min_block_size = stream.stream_info.max_block_size;
}

template <class SourceT>
component::Stream new_stream_for(const config::Encoder& config, const SourceT& src) {
  try {
    config.verify();
  } catch (const error::VerifyError& e) {
    throw error::EncodeError(error::EncodeError::Config, e.what());
  }
  const size_t nch = src.channels();
  const size_t bps = src.bits_per_sample();
  if (nch < 1 || nch > constant::MAX_CHANNELS || bps < constant::MIN_BITS_PER_SAMPLE ||
      bps > constant::MAX_BITS_PER_SAMPLE)
    throw error::EncodeError(error::EncodeError::Config, "stream_info: channels / bits_per_sample out of range");
  component::Stream stream;
  stream.stream_info.sample_rate = src.sample_rate();
  stream.stream_info.channels = nch;
  stream.stream_info.bits_per_sample = bps;
  return stream;
}
}  // namespace detail

// encode_with_fixed_block_size, src/coding.rs:645-700: reads the whole source and codes all full-size frames in ONE
// GPU batch (the tail frame, if shorter, in a second one): the reference's per-frame controller and bit writer on the
// device.
template <class SourceT>
component::Stream encode_with_fixed_block_size(const config::Encoder& config, SourceT src, size_t block_size,
                                               HipContext& gpu) {
  component::Stream stream = detail::new_stream_for(config, src);
  const size_t nch = src.channels(), bps = src.bits_per_sample();
  std::vector<source::FrameBuf> bufs = detail::drain_source(src, block_size, nch, bps, stream);
  std::vector<const source::FrameBuf*> run;
  run.reserve(bufs.size());
  for (const source::FrameBuf& fb : bufs) run.push_back(&fb);
  for (component::Frame& f : detail::encode_frame_run(config, run, 0, 1, nch, bps, src.sample_rate(), gpu))
    stream.add_frame(std::move(f));
  detail::finalize_block_sizes(stream);
  return stream;
}

// Sink that stores encoding results by serial id and hands them out in id order: ParSink,
// src/par.rs:67-95 (a BTreeMap behind a Mutex there, a std::map behind a std::mutex here).
template <class T>
class ParSink {
 public:
  void push(size_t idx, T element) {
    std::lock_guard<std::mutex> lock(mutex_);
    data_.emplace(idx, std::move(element));
  }
  template <class F>
  void finalize(F f) {  // empties the sink, calling f in the order of the serial id
    std::map<size_t, T> data;
    {
      std::lock_guard<std::mutex> lock(mutex_);
      data.swap(data_);
    }
    for (auto& kv : data) f(std::move(kv.second));
  }

 private:
  std::mutex mutex_;
  std::map<size_t, T> data_;
};

// encode_with_fixed_block_size over several GPUs -- the shape of the reference's par-mode encoder
// (src/par.rs:355-449) with the worker pool replaced by the node's GPUs: one host thread and one
// handle per device (a handle is single-threaded, like the reference's thread-local scratch), stream
// frame f goes to device f mod G (BASELINE config 4's round-robin; frames are independent),
// every device analyses and packs its frames as one batch with the right frame numbers in the headers
// (first = r, step = G), and a ParSink puts the finished frames back into frame-number order.
// Errors raised on a worker thread are re-thrown here after all workers have been joined.
template <class SourceT>
component::Stream encode_with_fixed_block_size(const config::Encoder& config, SourceT src, size_t block_size,
                                               std::vector<HipContext>& gpus) {
  if (gpus.empty()) throw error::EncodeError(error::EncodeError::Device, "no GPU context given");
  component::Stream stream = detail::new_stream_for(config, src);
  const size_t nch = src.channels(), bps = src.bits_per_sample(), rate = src.sample_rate();
  std::vector<source::FrameBuf> bufs = detail::drain_source(src, block_size, nch, bps, stream);
  const size_t G = gpus.size();
  ParSink<component::Frame> sink;
  std::vector<std::exception_ptr> failures(G);
  std::vector<std::thread> workers;
  workers.reserve(G);
  for (size_t r = 0; r < G; ++r) {
    workers.emplace_back([&, r] {
      try {
        std::vector<const source::FrameBuf*> run;
        for (size_t f = r; f < bufs.size(); f += G) run.push_back(&bufs[f]);
        for (component::Frame& fr : detail::encode_frame_run(config, run, r, G, nch, bps, rate, gpus[r])) {
          const size_t number = fr.frame_number;
          sink.push(number, std::move(fr));
        }
      } catch (...) {
        failures[r] = std::current_exception();
      }
    });
  }
  for (std::thread& t : workers) t.join();
  for (const std::exception_ptr& e : failures)
    if (e) std::rethrow_exception(e);
  sink.finalize([&](component::Frame f) { stream.add_frame(std::move(f)); });
  detail::finalize_block_sizes(stream);
  return stream;
}

// Frame::decode (src/component/decode.rs:55-110) for a run of frames on the GPU: frame f is lengths[f] bytes at
// bytes + offsets[f] (host memory).  Each result is the frame's samples interleaved as Frame::decode lays them out
// (decode.rs:101-107), or empty with the frame's FLACENC_HIP_DECODE_* bits in `status`.
struct DecodedFrame {
  uint32_t status = 0;
  uint64_t number = 0;
  size_t block_size = 0;
  std::vector<int32_t> samples;  // interleaved, block_size * channels
};

inline std::vector<DecodedFrame> decode_frames(HipContext& gpu, const uint8_t* bytes, size_t n_bytes,
                                               const std::vector<uint64_t>& offsets,
                                               const std::vector<uint32_t>& lengths, size_t channels,
                                               size_t bits_per_sample, size_t max_block_size) {
  const size_t n = offsets.size();
  if (lengths.size() != n) throw std::invalid_argument("decode_frames: offsets and lengths differ in length");
  std::vector<int32_t> rows(n * channels * max_block_size);
  std::vector<uint32_t> block_sizes(n), status(n);
  std::vector<uint64_t> numbers(n);
  const int rc = flacenc_hip_decode_frames(gpu.get(), bytes, n_bytes, offsets.data(), lengths.data(), n,
                                           static_cast<uint32_t>(channels), static_cast<uint32_t>(bits_per_sample),
                                           static_cast<uint32_t>(max_block_size), rows.data(), max_block_size,
                                           block_sizes.data(), numbers.data(), status.data(), FLACENC_HIP_MEM_HOST);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  std::vector<DecodedFrame> out(n);
  for (size_t f = 0; f < n; ++f) {
    out[f].status = status[f];
    if (status[f]) continue;
    out[f].number = numbers[f];
    out[f].block_size = block_sizes[f];
    out[f].samples.resize(block_sizes[f] * channels);
    const int32_t* base = rows.data() + f * channels * max_block_size;
    for (size_t c = 0; c < channels; ++c)
      for (size_t t = 0; t < block_sizes[f]; ++t) out[f].samples[t * channels + c] = base[c * max_block_size + t];
  }
  return out;
}

// `flacenc decode` for a whole stream: the verified chain of frames from bytes[0] (host memory, frames only) to packed
// interleaved little-endian PCM of ceil(bits_per_sample / 8) bytes per sample -- the bytes the STREAMINFO MD5 is defined
// over (src/source.rs:406-428) -- through flacenc_hip_decode_pcm.  out[0 .. samples * channels * width) is written and
// nothing behind it; after FLACENC_HIP_DECODE_NO_ROOM a second call on bytes + consumed continues the stream.
struct DecodedPcm {
  uint64_t frames = 0;
  uint64_t samples = 0;   // inter-channel samples written
  uint64_t consumed = 0;  // bytes of input: the start of the frame the call stopped at, or n_bytes
  uint32_t stop = 0;      // 0, FLACENC_HIP_DECODE_NO_ROOM, FLACENC_HIP_DECODE_CHAIN or a frame's FLACENC_HIP_DECODE_* bits
};

inline DecodedPcm decode_pcm(HipContext& gpu, const uint8_t* bytes, size_t n_bytes, size_t channels,
                             size_t bits_per_sample, size_t max_block_size, uint8_t* out, size_t out_capacity) {
  uint64_t totals[4] = {0, 0, 0, 0};
  const int rc = flacenc_hip_decode_pcm(gpu.get(), bytes, n_bytes, static_cast<uint32_t>(channels),
                                        static_cast<uint32_t>(bits_per_sample), static_cast<uint32_t>(max_block_size),
                                        static_cast<uint32_t>((bits_per_sample + 7) / 8), out, out_capacity, totals);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  DecodedPcm r;
  r.frames = totals[0];
  r.samples = totals[1];
  r.consumed = totals[2];
  r.stop = static_cast<uint32_t>(totals[3]);
  return r;
}

// A library of short files in one call (flacenc_hip_decode_streams on host memory): stream s is bytes[offset, offset +
// n_bytes) and decodes into out[out_offset, out_offset + out_capacity); the result for each is what decode_pcm gives for
// it alone.  Throws when the device fails and when the batch holds more frames than max_frames (nothing was written
// then; call again with more).
inline std::vector<DecodedPcm> decode_streams(HipContext& gpu, const uint8_t* bytes, size_t n_bytes,
                                              const std::vector<flacenc_hip_stream_desc>& streams, size_t max_frames,
                                              uint8_t* out, size_t out_bytes) {
  std::vector<uint64_t> totals(4 * streams.size() + 4, 0);
  uint64_t call[2] = {0, 0};
  const flacenc_hip_stream_desc none{};
  const int rc = flacenc_hip_decode_streams(gpu.get(), bytes, n_bytes, streams.empty() ? &none : streams.data(),
                                            streams.size(), max_frames, out, out_bytes, totals.data(), call,
                                            FLACENC_HIP_MEM_HOST);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  if (call[0] & FLACENC_HIP_INDEX_ERROR)
    throw error::EncodeError(error::EncodeError::Device, "decode_streams: more frames than max_frames");
  std::vector<DecodedPcm> r(streams.size());
  for (size_t s = 0; s < streams.size(); ++s) {
    r[s].frames = totals[4 * s];
    r[s].samples = totals[4 * s + 1];
    r[s].consumed = totals[4 * s + 2];
    r[s].stop = static_cast<uint32_t>(totals[4 * s + 3]);
  }
  return r;
}

// Seeking (flacenc_hip_decode_ranges on host memory): range r asks for samples [first_sample, first_sample + n_samples)
// of stream `stream`'s span -- positions count from the first sample of the span's first frame -- into out[out_offset ..).
// Only the frames the ranges touch are decoded.  The streams' out_offset and out_capacity are not looked at.  Throws when
// the device fails and when the chains or the ranges hold more frames than max_frames (nothing was written then).
struct DecodedRange {
  uint64_t samples = 0;      // inter-channel samples written
  uint32_t stop = 0;         // 0: all of them; the stream's stop reason, or FLACENC_HIP_DECODE_RANGE_END
  uint64_t seek_offset = 0;  // a seek point: the byte offset in the span, and the position, of the frame that holds
  uint64_t seek_sample = 0;  // first_sample
};

inline std::vector<DecodedRange> decode_ranges(HipContext& gpu, const uint8_t* bytes, size_t n_bytes,
                                               const std::vector<flacenc_hip_stream_desc>& streams,
                                               const std::vector<flacenc_hip_range_desc>& ranges, size_t max_frames,
                                               uint8_t* out, size_t out_bytes) {
  std::vector<uint64_t> totals(4 * ranges.size() + 4, 0);
  uint64_t call[2] = {0, 0};
  const flacenc_hip_stream_desc none{};
  const flacenc_hip_range_desc no_range{};
  const int rc = flacenc_hip_decode_ranges(gpu.get(), bytes, n_bytes, streams.empty() ? &none : streams.data(),
                                           streams.size(), ranges.empty() ? &no_range : ranges.data(), ranges.size(),
                                           max_frames, out, out_bytes, totals.data(), call, FLACENC_HIP_MEM_HOST);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  if (call[0] & FLACENC_HIP_INDEX_ERROR)
    throw error::EncodeError(error::EncodeError::Device, "decode_ranges: more frames than max_frames");
  std::vector<DecodedRange> r(ranges.size());
  for (size_t i = 0; i < ranges.size(); ++i) {
    r[i].samples = totals[4 * i];
    r[i].stop = static_cast<uint32_t>(totals[4 * i + 1]);
    r[i].seek_offset = totals[4 * i + 2];
    r[i].seek_sample = totals[4 * i + 3];
  }
  return r;
}

// The MD5 digests of a batch of spans of host memory in one call (flacenc_hip_md5_spans): span i is bytes[offsets[i],
// offsets[i] + lengths[i]), its digest the 16 bytes at 16 * i of the result -- what STREAMINFO stores.  One lane of the
// device hashes one span: the call for the digests of many files, not of one (one span alone is faster on the host).
inline std::vector<uint8_t> md5_spans(HipContext& gpu, const uint8_t* bytes, size_t n_bytes,
                                      const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& lengths) {
  if (offsets.size() != lengths.size())
    throw error::EncodeError(error::EncodeError::Device, "md5_spans: offsets and lengths differ in size");
  std::vector<uint8_t> digests(16 * offsets.size() + 16, 0);
  const uint64_t none = 0;
  const uint8_t no_bytes = 0;
  const int rc = flacenc_hip_md5_spans(gpu.get(), bytes ? bytes : &no_bytes, n_bytes, offsets.empty() ? &none : offsets.data(),
                                       lengths.empty() ? &none : lengths.data(), offsets.size(), digests.data(),
                                       FLACENC_HIP_MEM_HOST);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  digests.resize(16 * offsets.size());
  return digests;
}

// decode_streams plus every stream's MD5 (flacenc_hip_decode_streams_md5): digests[16 * s ..] is the digest of the bytes
// the call wrote to stream s's slot, computed on the device before the PCM left it -- for a stream that decoded to its
// end (stop == 0) the value its STREAMINFO must hold.
inline std::vector<DecodedPcm> decode_streams_md5(HipContext& gpu, const uint8_t* bytes, size_t n_bytes,
                                                  const std::vector<flacenc_hip_stream_desc>& streams, size_t max_frames,
                                                  uint8_t* out, size_t out_bytes, std::vector<uint8_t>& digests) {
  std::vector<uint64_t> totals(4 * streams.size() + 4, 0);
  uint64_t call[2] = {0, 0};
  const flacenc_hip_stream_desc none{};
  digests.assign(16 * streams.size() + 16, 0);
  const int rc = flacenc_hip_decode_streams_md5(gpu.get(), bytes, n_bytes, streams.empty() ? &none : streams.data(),
                                                streams.size(), max_frames, out, out_bytes, totals.data(), call,
                                                FLACENC_HIP_MEM_HOST, digests.data());
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  if (call[0] & FLACENC_HIP_INDEX_ERROR)
    throw error::EncodeError(error::EncodeError::Device, "decode_streams_md5: more frames than max_frames");
  digests.resize(16 * streams.size());
  std::vector<DecodedPcm> r(streams.size());
  for (size_t s = 0; s < streams.size(); ++s) {
    r[s].frames = totals[4 * s];
    r[s].samples = totals[4 * s + 1];
    r[s].consumed = totals[4 * s + 2];
    r[s].stop = static_cast<uint32_t>(totals[4 * s + 3]);
  }
  return r;
}

// The way there for a library of short files (flacenc_hip_encode_streams on host memory): stream s is the packed PCM
// pcm[offset, offset + total_samples * channels * bytes_per_sample) and its frames go to out[out_offset, out_offset +
// out_capacity) -- exactly the bytes flacenc_hip_encode_pcm gives for it alone, frame numbers from 0.  frame_lengths gets
// every frame's length, stream after stream; a stream whose slot was too small holds the whole frames that fit and says
// so (no_room).  Their STREAMINFO digests come from md5_spans over the same PCM spans.
struct EncodedStream {
  uint64_t frames = 0;        // frames written to the slot
  uint64_t bytes = 0;         // bytes written
  uint64_t first_length = 0;  // index of the stream's first entry in frame_lengths
  bool no_room = false;       // FLACENC_HIP_ENCODE_NO_ROOM: frames behind `frames` did not fit
};

inline std::vector<EncodedStream> encode_streams(HipContext& gpu, const flacenc_hip_frame_config& cfg, const uint8_t* pcm,
                                                 size_t pcm_bytes, const std::vector<flacenc_hip_pcm_stream_desc>& streams,
                                                 size_t block_size, uint8_t* out, size_t out_bytes,
                                                 std::vector<uint32_t>& frame_lengths) {
  const flacenc_hip_pcm_stream_desc none{};
  const flacenc_hip_pcm_stream_desc* table = streams.empty() ? &none : streams.data();
  const size_t n_frames = flacenc_hip_encode_streams_frames(table, streams.size(), static_cast<uint32_t>(block_size));
  frame_lengths.assign(n_frames + 1, 0);
  std::vector<uint64_t> totals(4 * streams.size() + 4, 0);
  uint64_t call[2] = {0, 0};
  const uint8_t no_bytes = 0;
  uint8_t no_out = 0;
  const int rc = flacenc_hip_encode_streams(gpu.get(), &cfg, pcm ? pcm : &no_bytes, pcm_bytes, table, streams.size(),
                                            static_cast<uint32_t>(block_size), out ? out : &no_out, out_bytes,
                                            frame_lengths.data(), n_frames, totals.data(), call, FLACENC_HIP_MEM_HOST);
  if (rc != FLACENC_HIP_OK) throw error::EncodeError(error::EncodeError::Device, flacenc_hip_last_error(gpu.get()));
  frame_lengths.resize(n_frames);
  std::vector<EncodedStream> r(streams.size());
  for (size_t s = 0; s < streams.size(); ++s) {
    r[s].frames = totals[4 * s];
    r[s].bytes = totals[4 * s + 1];
    r[s].first_length = totals[4 * s + 2];
    r[s].no_room = totals[4 * s + 3] == FLACENC_HIP_ENCODE_NO_ROOM;
  }
  return r;
}

}  // namespace flacenc
#endif  // FLACENC_HOST_FLACENC_HPP_
