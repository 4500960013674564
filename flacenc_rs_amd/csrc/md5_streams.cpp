// md5_streams.cpp -- MD5 digests of a batch of byte spans on the device: md5_spans_kernel, its launcher and
// flacenc_hip_md5_spans.
//
// MD5 is serial inside one message and independent across messages, so one LANE hashes one span: a workgroup is one
// wave of 64 spans, and the waves of a small batch spread over the CUs.  A lane keeps the state (4 words), the 16
// message words of the block it is hashing and the 16 + 1 aligned dwords of the block behind it in registers; the next
// block's loads are issued before the current block's 64 steps so that their latency hides behind the arithmetic (a
// small batch has one wave per CU and nothing else to switch to).  No LDS.
//
// Reads.  Lane i reads bytes [offset, offset + length) of `bytes` and nothing else, whatever the alignment of its
// start:
//   * the span's first aligned dword is assembled from its own bytes (the bytes in front of the span are another
//     span's or nobody's);
//   * a whole 64-byte block whose 17 aligned dwords all lie inside the span is read as dwords and brought into place
//     with a byte funnel shift (v_alignbyte_b32; shift 0 for an aligned start);
//   * every other block -- the last whole ones where the 17th dword would reach past the span, and the one or two
//     padded blocks -- is assembled bytewise by md5core::md5_pad_word, which asks for bytes of the span only.
// The lanes of a wave hash spans of unequal length: each loops over its own blocks, so the wave runs until its longest
// span is done and finished lanes sit masked off; they issue no load and no store.  flacenc_hip_md5_spans therefore hands
// the spans to the lanes in descending length order (`slot` says where a lane's digest goes), so that the spans of a wave
// are of similar length; flacenc_hip_decode_streams_md5, whose lengths exist on the device only, keeps stream order.
#include <algorithm>
#include <numeric>

#include "api_internal.h"
#include "md5_core.h"

namespace flacenc_hip {
namespace {

// the 16 message words of a block from 17 consecutive aligned dwords that start `a` bytes in front of it
#define MD5_FUNNEL(j) m[j] = __builtin_amdgcn_alignbyte(D[(j) + 1], D[j], a)
#define MD5_PAD(j) m[j] = md5core::md5_pad_word(at, pos, n, j)
#define MD5_ALL16(X) \
  X(0); X(1); X(2); X(3); X(4); X(5); X(6); X(7); X(8); X(9); X(10); X(11); X(12); X(13); X(14); X(15)

// offsets[i * offset_stride]: the span table of flacenc_hip_md5_spans (stride 1) or the out_offset field of the
// decode_streams descriptors (stride 6 words).  lengths null: every span is empty.  slot null: lane i's digest is
// digest i; else it is digest slot[i] (a permutation).
__global__ void __launch_bounds__(64) md5_spans_kernel(const uint8_t* __restrict__ bytes,
                                                       const uint64_t* __restrict__ offsets, uint32_t offset_stride,
                                                       const uint64_t* __restrict__ lengths,
                                                       const uint32_t* __restrict__ slot, uint32_t n_spans,
                                                       uint8_t* __restrict__ digests) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_spans) return;
  const uint64_t n = lengths ? lengths[i] : 0;
  const uint8_t* p = bytes + (n ? offsets[static_cast<size_t>(i) * offset_stride] : 0);  // read for n != 0 only
  const uint32_t a = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 3u;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - a);  // dword k of q covers bytes 4k - a .. 4k - a + 3 of the span
  // blocks taken as dwords: block k needs q[16k + 1 .. 16k + 16] inside the span: 64 (k + 1) + 4 - a <= n
  const uint64_t n_fast = n + a >= 4 ? (n + a - 4) >> 6 : 0;
  const uint64_t n_blocks = md5core::md5_n_blocks(n);
  auto at = [p](uint64_t k) { return static_cast<uint32_t>(p[k]); };

  uint32_t state[4], m[16], D[17];
  md5core::md5_init(state);
#pragma unroll
  for (int j = 0; j < 17; ++j) D[j] = 0;
  if (n_fast) {
    // q[0] from the span's own first 4 - a bytes (n_fast != 0: there are at least 64 of them)
    for (uint32_t t = a; t < 4; ++t) D[0] |= static_cast<uint32_t>(p[t - a]) << (8u * t);
#pragma unroll
    for (int j = 1; j < 17; ++j) D[j] = q[j];
  }
  for (uint64_t k = 0; k < n_fast; ++k) {
    // The next block's dwords are asked for first and are in flight during this block's 64 steps; the scheduling
    // barriers keep the compiler from sinking the loads towards their use or hoisting the copies (and with them the
    // wait) to the front.  The last of these blocks asks for its own dwords again: inside the span like the first
    // time, and not used.
    const uint32_t* nq = q + 16 * (k + 1 < n_fast ? k + 1 : k);
    uint32_t N[17];
#pragma unroll
    for (int j = 1; j < 17; ++j) N[j] = nq[j];
    __builtin_amdgcn_sched_barrier(0);
    MD5_ALL16(MD5_FUNNEL);
    md5core::md5_block(state, m);
    __builtin_amdgcn_sched_barrier(0);
    D[0] = D[16];
#pragma unroll
    for (int j = 1; j < 17; ++j) D[j] = N[j];
  }
  // at most three more: a whole block whose 17th dword lies past the span, and the padded ones
  for (uint64_t k = n_fast; k < n_blocks; ++k) {
    const uint64_t pos = k << 6;
    MD5_ALL16(MD5_PAD);
    md5core::md5_block(state, m);
  }
  uint8_t* out = digests + 16 * static_cast<size_t>(slot ? slot[i] : i);
  if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
    for (int j = 0; j < 4; ++j) reinterpret_cast<uint32_t*>(out)[j] = state[j];
  } else {
    uint8_t d[16];
    md5core::md5_digest(state, d);
    for (int j = 0; j < 16; ++j) out[j] = d[j];
  }
}

#undef MD5_ALL16
#undef MD5_PAD
#undef MD5_FUNNEL

}  // namespace

hipError_t launch_md5_spans(const uint8_t* bytes, const uint64_t* offsets, uint32_t offset_stride,
                            const uint64_t* lengths, const uint32_t* slot, uint32_t n_spans, uint8_t* digests,
                            hipStream_t stream) {
  if (n_spans == 0) return hipSuccess;
  hipLaunchKernelGGL(md5_spans_kernel, dim3((n_spans + 63u) / 64u), dim3(64), 0, stream, bytes, offsets, offset_stride,
                     lengths, slot, n_spans, digests);
  return hipGetLastError();
}

}  // namespace flacenc_hip

using namespace flacenc_hip;

extern "C" int flacenc_hip_md5_spans(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes,
                                     const uint64_t* offsets, const uint64_t* lengths, size_t n_spans, uint8_t* digests,
                                     int memory_kind) {
  if (!h) return FLACENC_HIP_ERR_BAD_ARGUMENT;
  if ((memory_kind != FLACENC_HIP_MEM_HOST && memory_kind != FLACENC_HIP_MEM_DEVICE) || !bytes || !offsets || !lengths ||
      !digests || n_spans > md5core::MAX_SPANS || !md5core::spans_inside(offsets, lengths, n_spans, n_bytes)) {
    h->last_error = "md5_spans: null pointer, unknown memory kind, more than 2^24 spans or a span that reaches past n_bytes";
    return FLACENC_HIP_ERR_BAD_ARGUMENT;
  }
  if (n_spans == 0) return FLACENC_HIP_OK;
  const bool host = memory_kind == FLACENC_HIP_MEM_HOST;
  const uint32_t ns = static_cast<uint32_t>(n_spans);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  int rc;
  // the span table (offsets | lengths | slots) through pinned staging; the digests behind it in the same scratch
  const size_t table_bytes = n_spans * 20, digest_bytes = n_spans * 16;
  if ((rc = ensure_pinned(h, h->pin_meta, &h->pin_meta_cap, table_bytes)) != FLACENC_HIP_OK) return rc;
  if ((rc = ensure(h, h->d_md5, a256(table_bytes) + digest_bytes)) != FLACENC_HIP_OK) return rc;
  uint64_t* p_table = static_cast<uint64_t*>(h->pin_meta[1]);
  uint32_t* p_slot = reinterpret_cast<uint32_t*>(p_table + 2 * n_spans);
  // lane i takes span p_slot[i]: descending length, ties in table order; a table that descends already stays as it is
  std::iota(p_slot, p_slot + n_spans, 0u);
  if (!std::is_sorted(lengths, lengths + n_spans, [](uint64_t a, uint64_t b) { return a > b; }))
    std::stable_sort(p_slot, p_slot + n_spans, [lengths](uint32_t a, uint32_t b) { return lengths[a] > lengths[b]; });
  for (size_t i = 0; i < n_spans; ++i) {
    p_table[i] = offsets[p_slot[i]];
    p_table[n_spans + i] = lengths[p_slot[i]];
  }
  uint64_t* d_table = static_cast<uint64_t*>(h->d_md5.ptr);
  const uint32_t* d_slot = reinterpret_cast<const uint32_t*>(d_table + 2 * n_spans);
  uint8_t* d_digests = host ? static_cast<uint8_t*>(h->d_md5.ptr) + a256(table_bytes) : digests;
  const uint8_t* d_bytes = bytes;
  const void* src = bytes;
  if (host && n_bytes) {
    if ((rc = ensure(h, h->d_dec_io, static_cast<size_t>(n_bytes) + 16)) != FLACENC_HIP_OK) return rc;
    d_bytes = static_cast<const uint8_t*>(h->d_dec_io.ptr);
    if (!is_pinned(bytes)) {  // pageable: through pinned staging on the handle's host threads
      if ((rc = ensure_pinned(h, h->pin_in, &h->pin_in_cap, static_cast<size_t>(n_bytes))) != FLACENC_HIP_OK) return rc;
      if ((rc = ensure_copy_pool(h, "md5_spans")) != FLACENC_HIP_OK) return rc;
      h->copy_pool->copy(h->pin_in[0], bytes, static_cast<size_t>(n_bytes));
      src = h->pin_in[0];
    }
  }
  int result = FLACENC_HIP_OK;
  hipError_t err = hipMemcpyAsync(d_table, p_table, table_bytes, hipMemcpyHostToDevice, st);
  if (err == hipSuccess && host && n_bytes)
    err = hipMemcpyAsync(h->d_dec_io.ptr, src, static_cast<size_t>(n_bytes), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = launch_md5_spans(d_bytes, d_table, 1, d_table + n_spans, d_slot, ns, d_digests, st);
  if (err == hipSuccess && host)
    err = hipMemcpyAsync(h->pin_meta[0], d_digests, digest_bytes, hipMemcpyDeviceToHost, st);
  if (err != hipSuccess) {
    set_error(h, "md5_spans", err);
    result = FLACENC_HIP_ERR_DEVICE;
  }
  // the handle's stream is drained before the call returns, also behind an error
  const hipError_t sync = hipStreamSynchronize(st);
  if (result == FLACENC_HIP_OK && sync != hipSuccess) {
    set_error(h, "md5_spans: hipStreamSynchronize", sync);
    result = FLACENC_HIP_ERR_DEVICE;
  }
  if (result == FLACENC_HIP_OK && host) std::memcpy(digests, h->pin_meta[0], digest_bytes);
  return result;
}
