// cdpr_readout.hpp - where the columns a getter hands out live: one table per layout, plain data for host and device.  A BLOCK is one
// robot-major array of the C-ABI ([B][width]); a block's columns are 16-bit source codes into ONE buffer of the handle, its state or
// its observable image:
//   float4 slot rows (fp32 handles):   code = slot * 4 + component, element ((code >> 2) * stride + r) * 4 + (code & 3) floats
//   double rows (precision = 64):      code = row,                  element code * stride + r doubles
// The gather kernel, the decoders of a recorded image and cdpr_set_platform_state* read these two functions and nothing else; the
// device-side readers of cdpr_env.hpp and cdpr_done.hpp keep their own row constants.
#pragma once
#include <cstddef>
#include "cdpr_step_kernel.hpp"
#include "cdpr_step_kernel_f64.hpp"

namespace cdpr {

enum ReadBlock {
  kReadPosition, kReadVelocity, kReadEffort, kReadPose, kReadTwist,  // the published step (observable image), in the image's order
  kReadRawPose, kReadRawTwist, kReadFkPose,                          // state
  kReadFkResidual, kReadFkIterations, kReadFlags,                    // observable image
};

static_assert(kReadPosition == 0 && kReadVelocity == 1 && kReadEffort == 2, "the joint blocks are the joint fields 0, 1, 2 (slot_columns, row_columns)");

struct BlockColumns {
  bool state;     // the block lives in the state buffer (else: the observable image)
  uint32_t width;
  uint16_t code[CDPR_MAX_CABLES];
};
static_assert(CDPR_MAX_CABLES >= 7u, "BlockColumns: a pose of seven columns must fit");

inline BlockColumns column_run(bool state, uint32_t first, uint32_t width) {
  BlockColumns b{state, width, {}};
  for (uint32_t j = 0; j < width; ++j) b.code[j] = (uint16_t)(first + j);
  return b;
}

// fp32 handles.  Pose7 = slot 0 xyzw, slot 1 xyz; twist6 = slot 1 w, slot 2 xyzw, slot 3 x - of the state and of the image alike.
// State slot 3 yzw + slot 4 xyzw: the FK estimate (slot 4 exists with the FK stage only: without it the seed is its position).
// Image slot 3 y z w: FK residual, iteration count, flags (pack_flags); joint field f of cable i: slot 4 + f G + i / 4, component i % 4.
inline BlockColumns slot_columns(int block, uint32_t n, bool fk) {
  const uint32_t G = (uint32_t)joint_groups((int)n);
  switch (block) {
    case kReadPose: return column_run(false, 0, 7);
    case kReadTwist: return column_run(false, 7, 6);
    case kReadRawPose: return column_run(true, 0, 7);
    case kReadRawTwist: return column_run(true, 7, 6);
    case kReadFkPose: return column_run(true, 13, fk ? 7 : 3);
    case kReadFkResidual: return column_run(false, 13, 1);
    case kReadFkIterations: return column_run(false, 14, 1);
    case kReadFlags: return column_run(false, 15, 1);
    default: return column_run(false, 4 * (4 + (uint32_t)block * G), n);  // kReadPosition / Velocity / Effort = field 0 / 1 / 2
  }
}

// precision = 64 handles: the rows of cdpr_step_kernel_f64.hpp
inline BlockColumns row_columns(int block, uint32_t n) {
  switch (block) {
    case kReadPose: return column_run(false, kF64Pose, 7);
    case kReadTwist: return column_run(false, kF64Twist, 6);
    case kReadRawPose: return column_run(true, kF64Pose, 7);
    case kReadRawTwist: return column_run(true, kF64Twist, 6);
    case kReadFkPose: return column_run(true, kF64StateFk, 7);
    case kReadFkResidual: return column_run(false, kF64ObsResidual, 1);
    case kReadFkIterations: return column_run(false, kF64ObsIterations, 1);
    case kReadFlags: return column_run(false, kF64ObsFlags, 1);
    default: return column_run(false, kF64ObsJoint + (uint32_t)block * n, n);
  }
}

// the element of robot r a code stands for, in elements of the layout's type
template <typename T>
__host__ __device__ inline size_t read_element(uint32_t code, uint32_t stride, uint32_t r);
template <>
__host__ __device__ inline size_t read_element<float>(uint32_t code, uint32_t stride, uint32_t r) { return ((size_t)(code >> 2) * stride + r) * 4u + (code & 3u); }
template <>
__host__ __device__ inline size_t read_element<double>(uint32_t code, uint32_t stride, uint32_t r) { return (size_t)code * stride + r; }

// The gather's argument: up to five blocks, consecutive in `out` (block k: [batch][width[k]] from element off[k] on, its codes from
// code[col0[k]] on).  Values leave as float or double (a double source rounds once); a block of as_int leaves as int32 (iteration
// counts, flags: small exact integers).  done: the optional host-mapped completion word, see the kernel.
constexpr uint32_t kReadMaxBlocks = 5;
constexpr uint32_t kReadMaxColumns = 3u * CDPR_MAX_CABLES + 13u;  // three joint blocks of n columns, pose7, twist6
struct ReadoutArgs {
  // what every thread needs in front of its load, in the argument's first 64 B (a kernel waits for each cache line of its argument it
  // reads; HISTORY.md section 20: tried against a 0.5 - 1 us cost at one robot, which it did not measurably remove)
  const void* rows;
  void* out;
  uint32_t stride, total;            // total: elements of all blocks
  uint32_t off[kReadMaxBlocks - 1];  // element offset of block k + 1 in `out` (block 0 starts at 0)
  uint8_t width[kReadMaxBlocks], col0[kReadMaxBlocks];
  uint8_t nblocks;
  uint8_t as_int;                    // bit k: block k
  uint8_t out_double;
  // the tail's
  uint64_t* done;      // host-mapped completion word, or null
  uint32_t* arrivals;  // device counter, zero between launches
  uint64_t epoch;
  uint16_t code[kReadMaxColumns];
};
static_assert(offsetof(ReadoutArgs, done) <= 64, "ReadoutArgs: the gather's own fields fill the first cache line and no more");
static_assert(kReadMaxColumns <= 256u && CDPR_MAX_CABLES <= 255u && kReadMaxBlocks <= 8u, "ReadoutArgs: widths, first columns and block bits are bytes");
static_assert(sizeof(ReadoutArgs::code) == 2u * (3u * CDPR_MAX_CABLES + 13u), "ReadoutArgs: one code per output column at CDPR_MAX_CABLES cables");
static_assert(4u * (4u + 3u * ((CDPR_MAX_CABLES + 3u) / 4u)) <= 65536u && 16u + 3u * CDPR_MAX_CABLES <= 65536u, "a column code is 16 bits");
static_assert(CDPR_MAX_CABLES + 1u <= 24u, "pack_flags: the TD flag and one travel-limit bit per cable must stay exact in a float");

}  // namespace cdpr
