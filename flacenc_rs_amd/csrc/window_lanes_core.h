#ifndef FLACENC_HIP_WINDOW_LANES_CORE_H_
#define FLACENC_HIP_WINDOW_LANES_CORE_H_
// window_lanes_core.h -- the lane-major copy of the analysis window for blocks of 4096 samples, for the device (the
// fused 4096 kernel's phase 1 at four workgroups per CU, qlpc_wave_kernel_impl.h) and for the host (get_window_entry
// builds it; tests/host/window_lanes_test.cpp holds it equal to the time-major weights).
//
// Phase 1 of that kernel gives lane l the samples [64 l, 64 l + 64) and reads the weights in quads at the lane-relative
// offsets -12 (the halo of orders 10 / 12), -8, -4, 0, ..., 68 (the look-ahead fetch behind the lane's last step).  In
// the time-major table the 64 lanes of one such load are 256 bytes apart: 64 cache lines, 16 bytes used of each.  Here
// slot j holds the quad at offset 4 j - 12 of every lane, lane after lane: one load reads 1 KB contiguous (8 lines), at
// the table's base + the immediate 1024 j + the one lane-dependent term 16 lane.
//
//   entry (j, lane, i) = w[64 lane - 12 + 4 j + i],  j = 0..20, lane = 0..63, i = 0..3,
//                        at float index (64 j + lane) 4 + i; 0.0f where the sample number is outside [0, 4096)
//
// (what the padded time-major table returns there: 32 zeros in front of it, 16 behind).  21 slots x 1 KB = 21 KB.
#include <stdint.h>

#if defined(__HIPCC__)
#define FLACENC_WLANES_HD __host__ __device__ __forceinline__
#else
#define FLACENC_WLANES_HD inline
#endif

namespace flacenc_hip {
namespace window_lanes {

constexpr int kBlock = 4096;        // the block size the table exists for
constexpr int kLanes = 64;
constexpr int kPerLane = 64;        // samples per lane
constexpr int kFirstOffset = -12;   // lane-relative offset of slot 0
constexpr int kSlots = 21;          // offsets -12 .. 68
constexpr int kSlotFloats = kLanes * 4;
constexpr int kFloats = kSlots * kSlotFloats;  // 5376 floats = 21 KB

// the slot of the quad at lane-relative offset `off` (a multiple of 4, -12 <= off <= 68)
FLACENC_WLANES_HD constexpr int slot_of(int off) { return (off - kFirstOffset) >> 2; }
// float index of entry (j, lane, i)
FLACENC_WLANES_HD constexpr int index(int j, int lane, int i) { return ((j * kLanes + lane) << 2) + i; }
// the sample number entry (j, lane, i) holds the weight of (outside [0, kBlock): the entry is 0.0f)
FLACENC_WLANES_HD constexpr int sample_of(int j, int lane, int i) { return kPerLane * lane + kFirstOffset + 4 * j + i; }

// out[kFloats] from the time-major weights w[0 .. kBlock)
inline void build(const float* w, float* out) {
  for (int j = 0; j < kSlots; ++j)
    for (int lane = 0; lane < kLanes; ++lane)
      for (int i = 0; i < 4; ++i) {
        const int t = sample_of(j, lane, i);
        out[index(j, lane, i)] = (t >= 0 && t < kBlock) ? w[t] : 0.0f;
      }
}

}  // namespace window_lanes
}  // namespace flacenc_hip
#endif
