// mirror_stream_tool.cpp -- runs the C++ host mirror (flacenc_rs_amd/host/flacenc.hpp) over a directory of cases that
// tests/test_gpu_host_mirror_stream.py wrote, in ONE process on one HipContext (plus up to three more on the same device
// for the several-handle cases), and writes for every case what the mirror gave: the stream's bytes or the exception, and
// a sidecar with every StreamInfo field and every frame's components.  Then it drives the mirror's way back
// (decode_frames, decode_pcm, decode_streams, decode_streams_md5, md5_spans) on the streams it just made.  It judges
// nothing: every comparison is the Python side's, against the CPU oracle.
//
//   <dir>/cases.txt      "case NAME", then "key value.." lines, then "end"; the case's PCM is <dir>/NAME.pcm
//                        (interleaved int32)
//   <dir>/NAME.flac      Stream::to_bytes()            |  <dir>/NAME.err   "kind\ntext" of the exception
//   <dir>/NAME.side      "info ..", per frame "frame ..", per subframe "sub ..", "roundtrip 0|1" (see write_side)
//   <dir>/wayback.txt    + .bin files: see way_back()
//
// A device error (EncodeError::Device outside the calls that must throw) ends the run with exit status 2 at once.
// Build + run: see tests/test_gpu_host_mirror_stream.py.
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "flacenc.hpp"

using namespace flacenc;

struct Case {
  std::string name;
  std::map<std::string, std::string> kv;
  std::vector<std::array<double, 4>> windows;  // type, alpha, start, end
  long num(const std::string& k) const {
    auto it = kv.find(k);
    if (it == kv.end()) {
      std::fprintf(stderr, "case %s: key %s missing\n", name.c_str(), k.c_str());
      std::exit(3);
    }
    return std::stol(it->second);
  }
  double real(const std::string& k) const {
    num(k);
    return std::stod(kv.at(k));
  }
};

struct Made {  // what the way back needs of a finished case
  std::string name;
  size_t channels, bps, block;
  std::vector<uint8_t> frames;  // the stream's bytes behind STREAMINFO
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lengths;
  size_t total;
};

static std::string g_dir;

static std::vector<Case> read_cases() {
  std::ifstream in(g_dir + "/cases.txt");
  if (!in) {
    std::fprintf(stderr, "no cases.txt in %s\n", g_dir.c_str());
    std::exit(3);
  }
  std::vector<Case> cases;
  std::string line;
  Case cur;
  bool open = false;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string key;
    if (!(ls >> key)) continue;
    if (key == "case") {
      cur = Case();
      ls >> cur.name;
      open = true;
    } else if (key == "end") {
      if (open) cases.push_back(cur);
      open = false;
    } else if (key == "win") {
      std::array<double, 4> w{};
      ls >> w[0] >> w[1] >> w[2] >> w[3];
      cur.windows.push_back(w);
    } else {
      std::string v;
      ls >> v;
      cur.kv[key] = v;
    }
  }
  return cases;
}

template <class T>
static std::vector<T> read_bin(const std::string& path) {
  std::vector<T> v;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(3);
  }
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize(size_t(sz) / sizeof(T));
  if (sz && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3);
  std::fclose(f);
  return v;
}

static void write_bin(const std::string& path, const void* data, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || (bytes && std::fwrite(data, 1, bytes, f) != bytes)) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    std::exit(3);
  }
  std::fclose(f);
}

static void write_text(const std::string& path, const std::string& text) { write_bin(path, text.data(), text.size()); }

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

// the handle's settings exactly as the case states them: every setter is called for every case
static void apply(HipContext& gpu, const Case& c) {
  gpu.set_sum_order(static_cast<HipContext::SumOrder>(c.num("sum_order")));
  gpu.set_order_search(c.num("order_search") != 0);
  gpu.set_window_search(c.num("window_search") != 0);
  gpu.set_order_guess(c.num("order_guess") != 0);
  gpu.set_precision_search(c.num("precision_search") != 0);
  gpu.set_order_guesses(static_cast<uint32_t>(c.num("order_guesses")));
  gpu.set_precision_floor(static_cast<uint32_t>(c.num("precision_floor")));
  std::vector<uint32_t> types(c.windows.size() + 1), starts(c.windows.size() + 1), ends(c.windows.size() + 1);
  std::vector<float> alphas(c.windows.size() + 1);
  for (size_t i = 0; i < c.windows.size(); ++i) {
    types[i] = static_cast<uint32_t>(c.windows[i][0]);
    alphas[i] = static_cast<float>(c.windows[i][1]);
    starts[i] = static_cast<uint32_t>(c.windows[i][2]);
    ends[i] = static_cast<uint32_t>(c.windows[i][3]);
  }
  gpu.set_lpc_windows(types.data(), alphas.data(), starts.data(), ends.data(), static_cast<uint32_t>(c.windows.size()));
}

static config::Encoder encoder_of(const Case& c) {
  config::Encoder e;
  e.block_size = size_t(c.num("block_size"));
  e.stereo_coding.use_leftside = c.num("use_leftside") != 0;
  e.stereo_coding.use_rightside = c.num("use_rightside") != 0;
  e.stereo_coding.use_midside = c.num("use_midside") != 0;
  config::SubFrameCoding& s = e.subframe_coding;
  s.use_constant = c.num("use_constant") != 0;
  s.use_fixed = c.num("use_fixed") != 0;
  s.use_lpc = c.num("use_lpc") != 0;
  s.fixed.max_order = size_t(c.num("fixed_max_order"));
  s.fixed.order_sel.type = c.num("fixed_order_sel") ? config::OrderSel::ApproxEnt : config::OrderSel::BitCount;
  s.fixed.order_sel.partitions = size_t(c.num("fixed_partitions"));
  s.qlpc.lpc_order = size_t(c.num("lpc_order"));
  s.qlpc.quant_precision = size_t(c.num("quant_precision"));
  s.qlpc.window.type = c.num("window_type") ? config::Window::Tukey : config::Window::Rectangle;
  s.qlpc.window.alpha = static_cast<float>(c.real("tukey_alpha"));
  s.prc.max_parameter = size_t(c.num("max_parameter"));
  return e;
}

// sidecar:  info  sample_rate channels bits min_block max_block min_frame max_frame total_samples md5(hex)
//           frame number block_size channel_assignment bytes
//           sub   kind(0 Constant, 1 Verbatim, 2 FixedLpc, 3 Lpc) bits order precision shift partition_order count_bits
//                 n_params params..
//           roundtrip 0|1   (every frame's decode_channels() equals the input)
static void write_side(const Case& c, const component::Stream& st, const std::vector<int32_t>& pcm, size_t nch) {
  std::ostringstream o;
  const component::StreamInfo& si = st.stream_info;
  o << "info " << si.sample_rate << ' ' << si.channels << ' ' << si.bits_per_sample << ' ' << si.min_block_size << ' '
    << si.max_block_size << ' ' << si.min_frame_size << ' ' << si.max_frame_size << ' ' << si.total_samples << ' '
    << hex(si.md5_digest, 16) << '\n';
  bool same = true;
  size_t pos = 0;
  for (const component::Frame& f : st.frames) {
    o << "frame " << f.frame_number << ' ' << f.block_size << ' ' << int(f.channel_assignment) << ' '
      << f.precomputed_bitstream.size() << '\n';
    for (const component::SubFrame& sf : f.subframes) {
      const component::Residual* r = nullptr;
      size_t kind = sf.index(), bits = 0, order = 0, precision = 0;
      int shift = 0;
      if (const auto* k = std::get_if<component::Constant>(&sf)) bits = k->bits_per_sample;
      if (const auto* v = std::get_if<component::Verbatim>(&sf)) bits = v->bits_per_sample;
      if (const auto* x = std::get_if<component::FixedLpc>(&sf)) {
        bits = x->bits_per_sample;
        order = x->order();
        r = &x->residual;
      }
      if (const auto* l = std::get_if<component::Lpc>(&sf)) {
        bits = l->bits_per_sample;
        order = l->order();
        precision = l->parameters.precision;
        shift = l->parameters.shift;
        r = &l->residual;
      }
      o << "sub " << kind << ' ' << bits << ' ' << order << ' ' << precision << ' ' << shift << ' '
        << (r ? int(r->partition_order) : 0) << ' ' << component::count_bits(sf) << ' ' << (r ? r->rice_params.size() : 0);
      if (r)
        for (uint8_t p : r->rice_params) o << ' ' << int(p);
      o << '\n';
    }
    const auto ch = f.decode_channels();
    same = same && ch.size() == nch && pos + f.block_size <= pcm.size() / nch;
    for (size_t k = 0; same && k < nch; ++k)
      for (size_t t = 0; same && t < f.block_size; ++t) same = ch[k].size() == f.block_size && ch[k][t] == pcm[(pos + t) * nch + k];
    pos += f.block_size;
  }
  same = same && pos == pcm.size() / nch;
  o << "roundtrip " << (same ? 1 : 0) << '\n';
  write_text(g_dir + "/" + c.name + ".side", o.str());
}

static void device_error(const std::string& where, const char* what) {
  std::fprintf(stderr, "device error in %s: %s\n", where.c_str(), what);
  std::exit(2);
}

// "threw KIND text" or what `f` returns
template <class F>
static std::string outcome(F f) {
  try {
    return f();
  } catch (const error::EncodeError& e) {
    static const char* kinds[] = {"Source", "Config", "Device"};
    return std::string("threw ") + kinds[e.kind] + " " + e.what();
  } catch (const std::exception& e) {
    return std::string("threw std::exception ") + e.what();
  }
}

static void way_back(HipContext& gpu, const std::vector<Made>& made) {
  std::ostringstream o;
  std::vector<uint8_t> all;  // the streams' frames back to back, one odd byte between them
  std::vector<flacenc_hip_stream_desc> descs;
  std::vector<std::vector<uint8_t>> single;
  size_t out_total = 0, frames_total = 0;
  try {
    for (const Made& m : made) {
      const size_t width = (m.bps + 7) / 8, full = m.total * m.channels * width;
      // decode_frames: <name>.df.bin holds every frame's interleaved int32 samples back to back
      std::vector<DecodedFrame> df =
          decode_frames(gpu, m.frames.data(), m.frames.size(), m.offsets, m.lengths, m.channels, m.bps, m.block);
      std::vector<int32_t> samples;
      for (const DecodedFrame& d : df) {
        o << "df " << m.name << ' ' << d.status << ' ' << d.number << ' ' << d.block_size << '\n';
        samples.insert(samples.end(), d.samples.begin(), d.samples.end());
      }
      write_bin(g_dir + "/" + m.name + ".df.bin", samples.data(), samples.size() * 4);
      // decode_pcm, the whole stream: <name>.dp.bin is the buffer with its 64 canary bytes of 0xCD behind
      std::vector<uint8_t> buf(full + 64, 0xCD);
      DecodedPcm r = decode_pcm(gpu, m.frames.data(), m.frames.size(), m.channels, m.bps, m.block, buf.data(), full);
      o << "dp " << m.name << ' ' << r.frames << ' ' << r.samples << ' ' << r.consumed << ' ' << r.stop << '\n';
      write_bin(g_dir + "/" + m.name + ".dp.bin", buf.data(), buf.size());
      single.emplace_back(buf.begin(), buf.begin() + full);
      // room for 1.5 frames, then the rest from bytes + consumed
      std::vector<uint8_t> b1(full + 64, 0xCD), b2(full + 64, 0xCD);
      const size_t room = (m.block * 3 / 2) * m.channels * width;
      DecodedPcm r1 = decode_pcm(gpu, m.frames.data(), m.frames.size(), m.channels, m.bps, m.block, b1.data(), room);
      o << "dp1 " << m.name << ' ' << r1.frames << ' ' << r1.samples << ' ' << r1.consumed << ' ' << r1.stop << ' ' << room << '\n';
      write_bin(g_dir + "/" + m.name + ".dp1.bin", b1.data(), b1.size());
      DecodedPcm r2{};
      if (r1.consumed <= m.frames.size())
        r2 = decode_pcm(gpu, m.frames.data() + r1.consumed, m.frames.size() - r1.consumed, m.channels, m.bps, m.block,
                        b2.data(), full);
      o << "dp2 " << m.name << ' ' << r2.frames << ' ' << r2.samples << ' ' << r2.consumed << ' ' << r2.stop << '\n';
      write_bin(g_dir + "/" + m.name + ".dp2.bin", b2.data(), b2.size());
      flacenc_hip_stream_desc d{};
      all.push_back(0xEE);
      d.offset = all.size();
      d.n_bytes = m.frames.size();
      all.insert(all.end(), m.frames.begin(), m.frames.end());
      d.out_offset = out_total;
      d.out_capacity = full;
      d.channels = static_cast<uint32_t>(m.channels);
      d.bits_per_sample = static_cast<uint32_t>(m.bps);
      d.max_block_size = static_cast<uint32_t>(m.block);
      d.bytes_per_sample = static_cast<uint32_t>(width);
      descs.push_back(d);
      out_total += full;
      frames_total += m.offsets.size();
    }
    // decode_streams / decode_streams_md5 over all of them in one buffer
    std::vector<uint8_t> out(out_total + 64, 0xCD);
    std::vector<DecodedPcm> rs = decode_streams(gpu, all.data(), all.size(), descs, frames_total, out.data(), out_total);
    for (size_t s = 0; s < rs.size(); ++s)
      o << "ds " << made[s].name << ' ' << rs[s].frames << ' ' << rs[s].samples << ' ' << rs[s].consumed << ' ' << rs[s].stop << '\n';
    write_bin(g_dir + "/streams.bin", out.data(), out.size());
    std::vector<uint8_t> out5(out_total + 64, 0xCD), digests;
    rs = decode_streams_md5(gpu, all.data(), all.size(), descs, frames_total, out5.data(), out_total, digests);
    for (size_t s = 0; s < rs.size(); ++s)
      o << "dsmd5 " << made[s].name << ' ' << rs[s].frames << ' ' << rs[s].samples << ' ' << rs[s].consumed << ' ' << rs[s].stop
        << ' ' << (digests.size() == 16 * rs.size() ? hex(&digests[16 * s], 16) : std::string("missing")) << '\n';
    write_bin(g_dir + "/streams_md5.bin", out5.data(), out5.size());
  } catch (const error::EncodeError& e) {
    device_error("the way back", e.what());
  }
  // max_frames one too small throws; an empty list returns empty
  std::vector<uint8_t> scratch(out_total + 64, 0xCD), dg;
  o << "ds_small " << outcome([&] {
    decode_streams(gpu, all.data(), all.size(), descs, frames_total - 1, scratch.data(), out_total);
    return std::string("returned");
  }) << '\n';
  o << "dsmd5_small " << outcome([&] {
    decode_streams_md5(gpu, all.data(), all.size(), descs, frames_total - 1, scratch.data(), out_total, dg);
    return std::string("returned");
  }) << '\n';
  const std::vector<flacenc_hip_stream_desc> none;
  o << "ds_empty " << outcome([&] {
    return "returned " + std::to_string(decode_streams(gpu, all.data(), all.size(), none, 4, scratch.data(), out_total).size());
  }) << '\n';
  o << "dsmd5_empty " << outcome([&] {
    const size_t n = decode_streams_md5(gpu, all.data(), all.size(), none, 4, scratch.data(), out_total, dg).size();
    return "returned " + std::to_string(n) + " " + std::to_string(dg.size());
  }) << '\n';
  // md5_spans: <dir>/md5.bin and the "offset length" lines of <dir>/md5_spans.txt
  const std::vector<uint8_t> blob = read_bin<uint8_t>(g_dir + "/md5.bin");
  std::vector<uint64_t> offs, lens;
  {
    std::ifstream in(g_dir + "/md5_spans.txt");
    uint64_t a, b;
    while (in >> a >> b) {
      offs.push_back(a);
      lens.push_back(b);
    }
  }
  const std::string got = outcome([&] {
    const std::vector<uint8_t> d = md5_spans(gpu, blob.data(), blob.size(), offs, lens);
    std::string s = "returned " + std::to_string(d.size() / 16);
    for (size_t i = 0; i + 16 <= d.size(); i += 16) s += " " + hex(&d[i], 16);
    return s;
  });
  if (got.rfind("threw", 0) == 0) device_error("md5_spans", got.c_str());
  o << "md5 " << got << '\n';
  o << "md5_empty " << outcome([&] {
    return "returned " + std::to_string(md5_spans(gpu, nullptr, 0, {}, {}).size());
  }) << '\n';
  o << "md5_sizes " << outcome([&] {
    md5_spans(gpu, blob.data(), blob.size(), offs, std::vector<uint64_t>(lens.begin(), lens.end() - 1));
    return std::string("returned");
  }) << '\n';
  write_text(g_dir + "/wayback.txt", o.str());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: mirror_stream_tool <case directory>\n");
    return 3;
  }
  g_dir = argv[1];
  const auto t0 = std::chrono::steady_clock::now();
  const std::vector<Case> cases = read_cases();
  HipContext gpu(0);
  std::vector<HipContext> pool;  // the several-handle cases' contexts: three more handles on the same device, four in all
  std::vector<Made> made;
  for (const Case& c : cases) {
    const size_t nch = size_t(c.num("channels")), bps = size_t(c.num("bits")), rate = size_t(c.num("rate"));
    const size_t block = size_t(c.num("block_size")), G = size_t(c.num("handles"));
    const std::vector<int32_t> pcm = read_bin<int32_t>(g_dir + "/" + c.name + ".pcm");
    const config::Encoder enc = encoder_of(c);
    std::string err_kind, err_text;
    try {
      component::Stream st;
      auto src = source::MemSource::from_samples(pcm, nch, bps, rate);
      if (G <= 1) {
        apply(gpu, c);
        st = encode_with_fixed_block_size(enc, src, block, gpu);
      } else {
        if (G > 3) {
          std::fprintf(stderr, "case %s: at most 3 handles beside the first\n", c.name.c_str());
          return 3;
        }
        while (pool.size() < 3) pool.emplace_back(0);
        std::vector<HipContext> gpus;
        for (size_t r = 0; r < G; ++r) {
          apply(pool[r], c);
          gpus.push_back(std::move(pool[r]));
        }
        std::exception_ptr thrown;
        try {
          st = encode_with_fixed_block_size(enc, src, block, gpus);
        } catch (...) {
          thrown = std::current_exception();
        }
        for (size_t r = 0; r < G; ++r) pool[r] = std::move(gpus[r]);
        if (thrown) std::rethrow_exception(thrown);
      }
      write_side(c, st, pcm, nch);
      const std::vector<uint8_t> bytes = st.to_bytes();
      write_bin(g_dir + "/" + c.name + ".flac", bytes.data(), bytes.size());
      if (c.num("wayback")) {
        Made m{c.name, nch, bps, block, std::vector<uint8_t>(bytes.begin() + 42, bytes.end()), {}, {}, pcm.size() / nch};
        uint64_t at = 0;
        for (const component::Frame& f : st.frames) {
          m.offsets.push_back(at);
          m.lengths.push_back(static_cast<uint32_t>(f.precomputed_bitstream.size()));
          at += f.precomputed_bitstream.size();
        }
        made.push_back(std::move(m));
      }
    } catch (const error::EncodeError& e) {
      if (e.kind == error::EncodeError::Device) device_error(c.name, e.what());
      err_kind = e.kind == error::EncodeError::Config ? "EncodeError::Config" : "EncodeError::Source";
      err_text = e.what();
    } catch (const error::VerifyError& e) {
      err_kind = "VerifyError";
      err_text = e.what();
    } catch (const std::exception& e) {
      err_kind = "std::exception";
      err_text = e.what();
    }
    if (!err_kind.empty()) write_text(g_dir + "/" + c.name + ".err", err_kind + "\n" + err_text + "\n");
    std::printf("%s: %s\n", c.name.c_str(), err_kind.empty() ? "stream" : err_kind.c_str());
    std::fflush(stdout);
  }
  if (!made.empty()) way_back(gpu, made);
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("mirror_stream_tool: %zu cases in %.2f s\n", cases.size(), secs);
  write_text(g_dir + "/done.txt", std::to_string(secs) + "\n");
  return 0;
}
