// variable_block.h -- launch interface of the block-size search's own kernels (variable_block.cpp).  The encoding of
// every candidate block is the fixed-blocking encode+pack call at that block size; what is here cuts the superblocks
// into the levels' frames, picks each superblock's tiling and writes the chosen frames with variable-blocking headers.
#ifndef FLACENC_HIP_VARIABLE_BLOCK_H_
#define FLACENC_HIP_VARIABLE_BLOCK_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace flacenc_hip {

// Where each level's packed frames and lengths live in scratch.  Level k has frames of block[k] = S >> k samples:
// frame i * 2^k + j is samples [j * block[k], (j + 1) * block[k]) of superblock i.  Level 0 also holds the tail frame
// (index n_full, tail samples) when the input does not end on a superblock boundary.
struct VbsLayout {
  uint32_t levels;
  uint32_t superblock;  // S
  uint32_t n_full;      // whole superblocks
  uint32_t tail;        // samples of the last, partial superblock (0: none)
  uint64_t first_sample;
  const uint8_t* pack;  // level k frame f at pack + pack_base[k] + f * pack_stride[k]
  const uint32_t* lens;  // level k frame f's fixed-blocking byte length at lens[len_base[k] + f]
  uint64_t pack_base[5];
  uint64_t pack_stride[5];
  uint32_t len_base[5];
};

// One chosen frame: where its fixed-blocking bytes are and what it becomes.
struct VbsChosen {
  uint64_t sample;  // sample number of its first sample (first_sample_number + offset)
  uint32_t level;
  uint32_t index;   // frame index inside its level
  uint32_t block;   // samples
  uint32_t pad;
};

// superblock i channel c samples [j b, (j + 1) b) -> row ((i 2^k + j) channels + c) of dst (dst_stride)
hipError_t launch_reblock(const int32_t* src, size_t src_stride, uint32_t n_full, uint32_t channels,
                          uint32_t superblock, uint32_t level, int32_t* dst, size_t dst_stride, hipStream_t stream);
// one lane per superblock (n_full + (tail != 0)): split mask and chosen-frame count of each
hipError_t launch_vbs_decide(const VbsLayout& l, uint32_t* masks, uint32_t* counts, hipStream_t stream);
// one lane per superblock: the chosen frames' records and variable-blocking lengths at their slots (first[i] + t,
// slots >= max_slots are dropped), the split masks to the caller (user_masks may be NULL)
hipError_t launch_vbs_emit(const VbsLayout& l, const uint32_t* masks, const uint32_t* counts, const uint64_t* first,
                           uint32_t max_slots, VbsChosen* chosen, uint32_t* vlen, uint32_t* user_masks,
                           hipStream_t stream);
// A workgroup per chosen frame: header rewritten, body moved to out + offsets[f], CRC-16 combined; offsets / lengths /
// block sizes to the caller.  frame_total[0] = frames, byte_total[0] = bytes; when either exceeds the caller's room
// nothing is written to out or the per-frame arrays and totals[0] carries FLACENC_HIP_VARIABLE_OVERFLOW.
hipError_t launch_rehead(const VbsLayout& l, const VbsChosen* chosen, const uint64_t* voff,
                         const uint64_t* frame_total, const uint64_t* byte_total, uint32_t max_slots, uint8_t* out,
                         uint64_t out_capacity, uint64_t* frame_offsets, uint32_t* frame_lengths,
                         uint32_t* frame_block_sizes, uint64_t max_frames, uint64_t* totals, hipStream_t stream);

}  // namespace flacenc_hip
#endif
