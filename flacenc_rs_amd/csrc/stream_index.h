// stream_index.h -- the frame index of the decoder (stream_index.cpp holds its kernels).  One pipeline -- candidates, skim,
// CRC-16, link, jump levels -- serves the single stream of flacenc_hip_index_frames (launch_index_frames, flac_decode.h)
// and the segmented index of a batch of FLAC streams, as flacenc_hip_decode_streams (flac_decode_streams.cpp) and
// flacenc_hip_decode_ranges (flac_decode_ranges.cpp) share it: on top of the pipeline one chain per stream, the scan of
// chain lengths, the verdict, every chain frame enumerated and the two scans over the frame sequence (PCM bytes, frames
// with a status).  flacenc_hip_recover_streams (flac_recover_streams.cpp) asks for the resynchronising form of the same
// index (Request::resync).  build() queues all of it on the handle's stream and synchronises nothing; what it leaves in device
// scratch (h->d_idx) is described by Index.  Behind it the header holds what the host sides of those two batch calls
// share and the index does not need itself: call_limits_ok, sort_by_channels and download_pcm.  Internal to the library.
#ifndef STREAM_INDEX_H_
#define STREAM_INDEX_H_

#include "api_internal.h"
#include "flac_decode_core.h"
#include "stream_batch_core.h"

namespace flacenc_hip {
namespace streamindex {

// counters (uint32): the candidates found, -, 1 when the call ends with FLACENC_HIP_INDEX_ERROR, the frames enumerated
enum : uint32_t { C_CANDS = 0, C_ERR = 2, C_FRAMES = 3 };
// meta (uint64), what the host reads back: frames, samples, the error flag, chain frames, candidates; from M_CLASS on
// the words of flacenc_hip_decode_ranges (the range-frames in front of the ranges of 1 .. 9 channels)
enum : uint32_t { M_FRAMES = 0, M_SAMPLES = 1, M_ERR = 2, M_CHAIN = 3, M_CANDS = 4, M_CLASS = 8, M_WORDS = 64 };

struct Request {
  const uint8_t* bytes;  // the caller's, host or device memory
  uint64_t n_bytes;
  const flacenc_hip_stream_desc* table;  // host memory, checked
  size_t n_streams;                      // > 0
  size_t max_frames;
  bool host;
  const char* who;            // the call's name, for the copy pool's error text
  size_t extra_words;         // 64-bit words behind `base` in the result block (device and pinned)
  size_t pinned_tail;         // bytes of pinned room behind the result block
  const void* extra_table;    // goes up with the descriptors in the same transfer (may be null)
  size_t extra_table_bytes;
  size_t extra_scratch;       // bytes of device scratch of the caller's own
  // flacenc_hip_recover_streams: every candidate's coded number is kept (Index::cand_number), and a stream's chain
  // resynchronises -- its root is the first verified candidate of the span, the frame behind a frame the first verified
  // candidate at or behind its end.  false: the verified chain from the span's first byte, the index as it has always been
  bool resync;
};

struct Index {
  // the result block: counters | meta[M_WORDS] | base[n_streams + 1] | extra[extra_words]; `result_words` 64-bit words
  // from `meta` on are what the caller downloads into h->pin_meta[0]
  uint32_t* counters;
  uint64_t *meta, *base, *extra;
  size_t result_words;
  const flacenc_hip_stream_desc* descs;  // the table on the device
  const uint32_t* perm;                  // slot -> stream, the table sorted by channel count
  const char* extra_table;               // the caller's table on the device (8-byte aligned)
  uint32_t slot_lo[10];                  // host: slots [slot_lo[c], slot_lo[c + 1]) hold the streams of c channels
  uint32_t classes;                      // host: the channel counts present
  uint32_t cap, levels;                  // the candidate table's size and its jump levels
  const uint8_t* d_bytes;                // the input on the device
  uint64_t* cand_pos;
  flacdec::FrameRec* recs;
  uint32_t* jump;
  uint32_t *s_root, *s_why, *s_accepted;
  uint64_t *s_end, *s_bytes;
  uint32_t *f_node, *f_slot;  // per chain frame m < counters[C_FRAMES]: its candidate, its slot
  uint64_t *pcm, *bad;        // exclusive scans over the frame sequence, [max_frames + 1]
  char* scratch;              // extra_scratch bytes, 256-byte aligned
  const uint64_t* cand_number;  // Request::resync only: per candidate, coded number << 1 | blocking bit
};

// plan: launches, synchronisations, transfers, channel classes of the call (plan[3] is set, the others are added to)
int build(flacenc_hip_handle* h, uint64_t* plan, const Request& rq, Index& ix);

// The single-workgroup scan of up to two arrays (b may be null) of n 64-bit words: out_x[i] = the sum of x[j] over
// j < i, out_x[n] the total.  One launch.  The batch encoder (encode_streams.cpp) uses it too.
hipError_t launch_scan2(const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out_a, uint64_t* out_b,
                        hipStream_t stream);
// the same over min(n, *n_dev) words, n_dev device memory
hipError_t launch_scan2_dev(const uint64_t* a, const uint64_t* b, uint64_t n, const uint32_t* n_dev, uint64_t* out_a,
                            uint64_t* out_b, hipStream_t stream);

// What the two batch calls refuse alike, in front of their tables: the memory kind and the stream, frame and n_bytes
// limits.
inline bool call_limits_ok(int memory_kind, size_t n_streams, size_t max_frames, uint64_t n_bytes) {
  return (memory_kind == FLACENC_HIP_MEM_HOST || memory_kind == FLACENC_HIP_MEM_DEVICE) &&
         n_streams <= streambatch::MAX_STREAMS && max_frames <= streambatch::MAX_FRAMES &&
         n_bytes <= (static_cast<uint64_t>(0xFFFFFFFFu) << 12);
}

// n items sorted by their channel count (channels_of(i) in 1..=8), stably: perm[slot] = item, slots [lo[c], lo[c + 1])
// hold the items of c channels.  Returns the number of channel counts present.
template <class ChannelsOf>
uint32_t sort_by_channels(size_t n, ChannelsOf channels_of, uint32_t lo[10], uint32_t* perm) {
  for (uint32_t c = 0; c < 10; ++c) lo[c] = 0;
  for (size_t i = 0; i < n; ++i) ++lo[channels_of(i) + 1];
  uint32_t classes = 0;
  for (uint32_t c = 1; c <= 8; ++c) {
    classes += lo[c + 1] != 0;
    lo[c + 1] += lo[c];
  }
  uint32_t at[9];
  for (uint32_t c = 1; c <= 8; ++c) at[c] = lo[c];
  for (size_t i = 0; i < n; ++i) perm[at[channels_of(i)]++] = static_cast<uint32_t>(i);
  return classes;
}

// The host-memory download of a batch call: pcm_bytes of packed PCM from d_out into pinned staging (h->pin_out[0]) in
// one transfer, counted in plan[2], with the copy pool ready to scatter it.
int download_pcm(flacenc_hip_handle* h, uint64_t* plan, const char* who, const uint8_t* d_out, uint64_t pcm_bytes);

// the handle's stream is drained before an error hands the handle back
struct Drain {
  flacenc_hip_handle* h;
  bool armed = true;
  ~Drain() {
    if (armed) (void)hipStreamSynchronize(h->stream);
  }
};

}  // namespace streamindex
}  // namespace flacenc_hip

#endif  // STREAM_INDEX_H_
