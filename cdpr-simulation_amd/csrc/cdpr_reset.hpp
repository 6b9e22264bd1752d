// cdpr_reset.hpp — model reset of chosen robots of a per-robot handle (cdpr_reset_robots[_device]): the robots of the mask go back
// to what cdpr_create / cdpr_reset leave for every robot - JointForceCalculator::reset() (JFC.h:69-73) plus the state Load leaves
// (PLG.cpp:153-157: Position mode, target 0) - at a pose and twist of the caller's; the world clock, the other robots and every
// pending command stay as they are; the robot's episode clock restarts (one dword store).  One kernel per record layout: the register-resident per-robot records (cdpr_step_kernel.hpp),
// the general path's record buffer with its hot rows (cdpr_general_step.hpp), the precision = 64 rows (cdpr_step_kernel_f64.hpp).
//
// As the latch kernels (cdpr_latch.hpp): one thread per robot, 256 per block, the mask byte read once, a robot outside the mask
// leaves at once (its pose and twist rows are never read).  Every slot row and dword row a reset robot writes is addressed
// row * stride + r: neighbouring reset robots coalesce and the rest of the wave moves nothing.  No LDS, no scratch.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_kernels.hpp"

namespace cdpr {

// what the three kernels share: who is reset and where to
struct ResetWhere {
  const uint8_t* mask;  // uint8[B]
  const float* pose;    // float[B][7], or nullptr = home
  const float* twist;   // float[B][6], or nullptr = zero
  float home[7];        // cdpr_config_t.home_pose
  uint32_t batch;
  uint32_t* episode_start;  // uint32[B]: the world step of the robot's last model reset (cdpr_get_episode_start, CDPR_DONE_TIMEOUT)
  uint32_t step;        // low word of cdpr_step_count at the call
};

// the robot's pose and twist: its rows of the caller's buffers, or home and zero
CDPR_DEV void reset_rows(const ResetWhere& w, uint32_t r, float (&p)[7], float (&t)[6]) {
#pragma unroll
  for (int c = 0; c < 7; ++c) p[c] = w.pose ? w.pose[(size_t)r * 7 + c] : w.home[c];
#pragma unroll
  for (int c = 0; c < 6; ++c) t[c] = w.twist ? w.twist[(size_t)r * 6 + c] : 0.f;
}

// fp32 handles, both paths: platform slots 0-3 (+ 4 with FK: the seed follows the pose, as cdpr_set_platform_state has it), the
// observable image before the first publish (the pose, zeros elsewhere: joint rows, twist, FK residual and iterations, flags), the
// `pid` debug row
struct ResetPlatform {
  float4* state;
  float4* obs;
  float* dbg;           // float[B][9], or nullptr
  size_t stride;
  uint32_t n_obs, fk;
};
CDPR_DEV void reset_platform(const ResetPlatform& a, uint32_t r, const float (&p)[7], const float (&t)[6]) {
  const size_t st = a.stride;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  a.state[0 * st + r] = make_float4(p[0], p[1], p[2], p[3]);
  a.state[1 * st + r] = make_float4(p[4], p[5], p[6], t[0]);
  a.state[2 * st + r] = make_float4(t[1], t[2], t[3], t[4]);
  a.state[3 * st + r] = make_float4(t[5], p[0], p[1], p[2]);
  if (a.fk) a.state[4 * st + r] = make_float4(p[3], p[4], p[5], p[6]);
  a.obs[0 * st + r] = make_float4(p[0], p[1], p[2], p[3]);
  a.obs[1 * st + r] = make_float4(p[4], p[5], p[6], 0.f);
  for (uint32_t s = 2; s < a.n_obs; ++s) a.obs[(size_t)s * st + r] = zero;
  if (a.dbg)
    for (int c = 0; c < CDPR_PID_DEBUG_AXES; ++c) a.dbg[(size_t)r * CDPR_PID_DEBUG_AXES + c] = 0.f;
}

// Register-resident per-robot records: the integral rows zero, meta = Position mode with call count 0 (the next Pid::update is the
// "first" and returns 0, Pid.cpp:123-126), the active target row zero.  The derivative ring needs no clearing: a call count of 0
// hides it until nbuf new samples have overwritten every slot the weights reach (cdpr_latch.hpp).
struct ResetFastArgs {
  ResetWhere who;
  ResetPlatform plat;
  uint8_t* meta;        // StepArgs::meta
  float* target;        // float[B][n]
  float4* hot;          // first integral row of the state: slot P + 5 * pairs
  uint32_t n, hot_rows;
};

static __global__ __launch_bounds__(256) void cdpr_reset_fast_kernel(const ResetFastArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= a.who.batch) return;
  if (!a.who.mask[r]) return;
  float p[7], t[6];
  reset_rows(a.who, r, p, t);
  reset_platform(a.plat, r, p, t);
  for (uint32_t g = 0; g < a.hot_rows; ++g) a.hot[(size_t)g * a.plat.stride + r] = make_float4(0.f, 0.f, 0.f, 0.f);
  a.meta[r] = (uint8_t)kMetaPosition;
  for (uint32_t i = 0; i < a.n; ++i) a.target[(size_t)r * a.n + i] = 0.f;
  a.who.episode_start[r] = a.who.step;
}

// General path: the robot's column of the whole record buffer - mLastPosition slots, both Pids' slots (region A) and rows (region
// B) of every cable: all-zero IS Pid::reset - and its own hot-row word cleared (region C, row 0: the stale H slots it stood for have
// just been zeroed, so nothing is flushed; the robots around it keep their hot rows); Position mode; its row of the three latched
// command buffers zero (the engine's own buffers: a per-robot handle latches by copy, never by pointer).
struct ResetGenArgs {
  ResetWhere who;
  ResetPlatform plat;
  uint8_t* mode;        // per-robot mode (0 Force, 1 Position, 2 Velocity)
  float* latched[3];    // float[B][n] per command kind
  float* rec;
  uint32_t rstride, n;
  GenLayout lay;
};

static __global__ __launch_bounds__(256) void cdpr_reset_gen_kernel(const ResetGenArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= a.who.batch) return;
  if (!a.who.mask[r]) return;
  float p[7], t[6];
  reset_rows(a.who, r, p, t);
  reset_platform(a.plat, r, p, t);
  const size_t rs = a.rstride;
  float4* const sa = reinterpret_cast<float4*>(a.rec) + r;
  for (int sl = 0; sl < a.lay.slots(); ++sl) sa[(size_t)sl * rs] = make_float4(0.f, 0.f, 0.f, 0.f);
  float* const rb = a.rec + (size_t)a.lay.slots() * rs * 4 + r;
  for (int row = 0; row < a.lay.rows(); ++row) rb[(size_t)row * rs] = 0.f;
  rb[(size_t)a.lay.rows() * rs] = 0.f;  // region C, row 0: the robot's hot-row word
  a.mode[r] = (uint8_t)kMetaPosition;   // (= UpdateMode::Position, JFC.h:35-37)
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (uint32_t i = 0; i < a.n; ++i) a.latched[k][(size_t)r * a.n + i] = 0.f;
  a.who.episode_start[r] = a.who.step;
}

// precision = 64: the double rows of pose, twist and FK estimate (a float pose becomes a double exactly); the integral rows
// 20 + (win + 1) i + win or, on HOLD handles, every cable's mLastPosition row and both Pids' records (f64_hold_row); meta; the active
// target row; the observable image and the `pid` debug row in double.
struct ResetF64Args {
  ResetWhere who;
  double home[7];       // cdpr_config_t.home_pose as it is (upload_home64), in place of who.home
  double* state;
  double* obs;
  double* dbg;          // double[B][9], or nullptr
  uint8_t* meta;
  float* target;        // float[B][n]
  size_t stride;
  uint32_t n;
  uint32_t hold;        // HOLD handles (both Pids of every cable behind the state rows)
  uint32_t hold_win;    // ... samples such a record's window holds (kHoldWin | kHoldWinLong)
  uint32_t win;         // prior errors kept per cable (kWin | kWinLong)
};

static __global__ __launch_bounds__(256) void cdpr_reset_f64_kernel(const ResetF64Args a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= a.who.batch) return;
  if (!a.who.mask[r]) return;
  float p[7], t[6];
  reset_rows(a.who, r, p, t);
  const size_t st = a.stride;
  double* const S = a.state + r;
  double* const O = a.obs + r;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const double pc = a.who.pose ? (double)p[c] : a.home[c];
    S[(size_t)(kF64Pose + c) * st] = pc;
    S[(size_t)(kF64StateFk + c) * st] = pc;
    O[(size_t)(kF64Pose + c) * st] = pc;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) S[(size_t)(kF64Twist + c) * st] = (double)t[c];
  for (int row = kF64Twist; row < f64_obs_rows((int)a.n); ++row) O[(size_t)row * st] = 0.0;
  if (a.hold) {
    const int rows = hold_cable_rows((int)a.hold_win);
    for (uint32_t i = 0; i < a.n; ++i) {
      double* const C = S + (size_t)(f64_hold_row((int)a.n, (int)i, 0, (int)a.hold_win) - 1) * st;  // mLastPosition, then the two Pids
      for (int row = 0; row < rows; ++row) C[(size_t)row * st] = 0.0;
    }
  } else {
    for (uint32_t i = 0; i < a.n; ++i) S[(size_t)(kF64StateCtrl + (a.win + 1u) * i + a.win) * st] = 0.0;
  }
  a.meta[r] = (uint8_t)kMetaPosition;
  for (uint32_t i = 0; i < a.n; ++i) a.target[(size_t)r * a.n + i] = 0.f;
  if (a.dbg)
    for (int c = 0; c < CDPR_PID_DEBUG_AXES; ++c) a.dbg[(size_t)r * CDPR_PID_DEBUG_AXES + c] = 0.0;
  a.who.episode_start[r] = a.who.step;
}

}  // namespace cdpr
