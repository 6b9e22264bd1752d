// cdpr_robot_records.hpp — what ONE robot of a per-robot handle owns, said once per record layout: the register-resident per-robot
// records (FastRecords, cdpr_step_kernel.hpp), the general path's record buffer with its hot rows (GenRecords,
// cdpr_general_step.hpp), the precision = 64 rows (F64Records, cdpr_step_kernel_f64.hpp).  The host builds a view from the handle
// (fast_records / gen_records / f64_records, cdpr_engine_internal.hpp: nowhere else), and everything that acts on chosen robots is
// made of the functions below, each written once per layout:
//   pid_reset    Pid::reset of one Pid of robot r - what entering a mode does (JFC.cpp:101-103,113-115)
//   latch_robot  a Joy batch reaching robot r (cdpr_set_*_command[_masked]; PLG.cpp:206-219 runs per model)
//   model_reset  robot r back to what cdpr_create leaves, at a pose and twist of the caller's (cdpr_reset_robots[_device])
//   take_over    robot r continues from where robot s is now, to the bit (cdpr_copy_robots[_device])
// The kernels themselves (cdpr_latch_*_kernel, cdpr_gen_flush_hot_kernel: cdpr_engine_launch.hip; cdpr_reset_*_kernel:
// cdpr_engine_reset.hip; cdpr_copy_*_kernel: cdpr_engine_copy.hip) are the thread's robot index, the verdict of `who` and one call,
// and sit beside their only launcher, so the library carries one copy of each.  A buffer indexed by robot that a handle gains is added
// to its view(s), to the builder and to these three functions - and to nothing else.
//
// One thread per robot, 256 per block; the mask byte / map entry is read once and a robot outside it leaves at once.  Every slot
// row and dword row is addressed row * stride + r: neighbouring chosen robots coalesce and the rest of the wave moves nothing.  No
// LDS, no scratch.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_step_kernel.hpp"
#include "cdpr_step_kernel_f64.hpp"
#include "cdpr_general_step.hpp"

namespace cdpr {

// ---------------------------------------------------------------------------------------------------------------- the three views

// fp32 handles, both paths: the platform's share of the state slot rows (slots 0-3, + 4 with FK) in front of every other, the
// observable image, the `pid` debug row
struct PlatRows {
  float4* state;
  float4* obs;
  float* dbg;           // float[B][9], or nullptr
  size_t stride;
  uint32_t n_state, n_obs, fk;
};

// Register-resident per-robot records: every robot keeps ONE Pid record, the active mode's (StepArgs::meta).
struct FastRecords {
  uint32_t batch, n;         // (first: a kernel's bounds test then finds the batch in the cache line of `who`'s mask or map pointer)
  PlatRows plat;             // n_state: platform, FK estimate, ring rows, integral rows
  float4* integral;          // first integral row of the state: slot P + 5 * pairs
  uint32_t integral_rows;
  uint8_t* meta;             // StepArgs::meta: mode, and the Pid call count in bits 2-7
  float* target;             // float[B][n]: the robots' active target rows (StepArgs::cmd of the PR kernels)
  uint32_t* episode_start;   // uint32[B]: the world step of the robot's last model reset (cdpr_get_episode_start, CDPR_DONE_TIMEOUT)
};

// General path: the robot's column of the record buffer - region A (float4 slots: mLastPosition, both Pids), region B (dword rows)
// and region C (its hot rows) - and its rows of the engine's own latched command buffers (a per-robot handle latches by copy, never
// by pointer).
struct GenRecords {
  uint32_t batch, n;
  PlatRows plat;             // n_state: the platform slots
  float* rec;
  GenLayout lay;
  uint8_t* mode;             // per-robot mode (0 Force, 1 Position, 2 Velocity)
  float* latched[3];         // float[B][n] per command kind
  uint32_t* episode_start;
};

// precision = 64: the double rows of the state column at whatever record width the handle has (plain rings, or the HOLD records
// behind them with their packed words), the double image and `pid` row.
struct F64Records {
  uint32_t batch, n;
  double* state;
  double* obs;
  double* dbg;               // double[B][9], or nullptr
  uint8_t* meta;
  float* target;             // float[B][n]
  uint32_t* episode_start;
  size_t stride;
  uint32_t state_rows, obs_rows;
  uint32_t hold;             // HOLD handles: both Pids of every cable live in their own rows behind the state rows (f64_hold_row)
  uint32_t hold_win;         // ... samples such a record's window holds (kHoldWin | kHoldWinLong)
  uint32_t win;              // prior errors kept per cable (kWin | kWinLong): the integral is row f64_integral_row(i, win)
  double home[7];            // cdpr_config_t.home_pose as it is (upload_home64)
};

// -------------------------------------------------------------------------------------------------------------------- Pid::reset

// The robot's single record: integral 0 (the caller's meta write makes the call count 0, so the next Pid::update is the "first" and
// returns 0, Pid.cpp:123-126).  The derivative ring needs no clearing: derive() returns 0 until nbuf new samples are in, and by
// then they have overwritten every slot the weights reach.
CDPR_DEV void pid_reset(const FastRecords& v, uint32_t r) {
  for (uint32_t g = 0; g < v.integral_rows; ++g) v.integral[(size_t)g * v.plat.stride + r] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Pid `which` (0 position, 1 velocity) of every cable: the robot's column of the Pid's slots and rows - all-zero IS Pid::reset
CDPR_DEV void pid_reset(const GenRecords& v, uint32_t r, int which) {
  const size_t rs = v.plat.stride;
  float4* const sa = reinterpret_cast<float4*>(v.rec) + (size_t)v.lay.block_a(which, 0) * rs + r;
  for (int sl = 0; sl < v.lay.pid_slots(); ++sl) sa[(size_t)sl * rs] = make_float4(0.f, 0.f, 0.f, 0.f);
  float* const rb = v.rec + (size_t)v.lay.slots() * rs * 4 + (size_t)v.lay.block_b(which, 0) * rs + r;
  for (int row = 0; row < v.lay.pid_rows(); ++row) rb[(size_t)row * rs] = 0.f;
}

// HOLD handles: Pid `which` of every cable - word, integral, window, stamps; else the robot's single record: the integral rows
CDPR_DEV void pid_reset(const F64Records& v, uint32_t r, int which) {
  double* const S = v.state + r;
  if (v.hold) {
    for (uint32_t i = 0; i < v.n; ++i)
      for (int row = 0; row < hold_pid_rows((int)v.hold_win); ++row) S[(size_t)(f64_hold_row((int)v.n, (int)i, which, (int)v.hold_win) + row) * v.stride] = 0.0;
  } else {
    for (uint32_t i = 0; i < v.n; ++i) S[(size_t)f64_integral_row((int)i, (int)v.win) * v.stride] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- latch

// A Joy batch of one command kind: its row becomes the robot's target, and entering the kind's mode from another one resets that
// mode's Pid.  setForce (JFC.h:92-95) resets nothing; leaving Force mode resets the Pid entered.
struct LatchWho {
  const uint8_t* mask;   // uint8[B], or nullptr = every robot
  const float* pending;  // float[B][n]
  uint32_t kind;         // CDPR_COMMAND_*
  uint32_t new_mode;     // kMetaForce / kMetaPosition / kMetaVelocity (= UpdateMode, JFC.h:35-37)
  int reset_pid;         // the Pid whose records the mode owns (0 position, 1 velocity); -1: none (setForce)
};
CDPR_DEV bool latch_wanted(const LatchWho& w, uint32_t batch, uint32_t r) { return r < batch && (!w.mask || w.mask[r]); }

// meta of a robot with one Pid record after the batch: `entered` says that the record has to be reset (call count 0)
CDPR_DEV uint32_t latch_meta(const LatchWho& w, uint32_t m, bool& entered) {
  entered = w.new_mode != kMetaForce && (m & kMetaModeMask) != w.new_mode;
  return w.new_mode == kMetaForce ? (m & ~kMetaModeMask) | kMetaForce : entered ? w.new_mode : m;
}

CDPR_DEV void latch_robot(const LatchWho& w, const FastRecords& v, uint32_t r) {
  for (uint32_t i = 0; i < v.n; ++i) v.target[(size_t)r * v.n + i] = w.pending[(size_t)r * v.n + i];
  bool entered;
  const uint32_t m = latch_meta(w, v.meta[r], entered);
  if (entered) pid_reset(v, r);
  v.meta[r] = (uint8_t)m;
}

CDPR_DEV void latch_robot(const LatchWho& w, const GenRecords& v, uint32_t r) {
  float* const latched = v.latched[w.kind];
  for (uint32_t i = 0; i < v.n; ++i) latched[(size_t)r * v.n + i] = w.pending[(size_t)r * v.n + i];
  if ((uint32_t)v.mode[r] != w.new_mode) {
    if (w.reset_pid >= 0) pid_reset(v, r, w.reset_pid);
    v.mode[r] = (uint8_t)w.new_mode;
  }
}

CDPR_DEV void latch_robot(const LatchWho& w, const F64Records& v, uint32_t r) {
  for (uint32_t i = 0; i < v.n; ++i) v.target[(size_t)r * v.n + i] = w.pending[(size_t)r * v.n + i];
  bool entered;
  const uint32_t m = latch_meta(w, v.meta[r], entered);
  if (entered) pid_reset(v, r, w.reset_pid);
  v.meta[r] = (uint8_t)m;
}

// The general path's hot rows (GenHot) written back: a robot with a valid word gets the H slots of its word's Pids as they stand and
// its word cleared.  Runs in front of anything that resets a Pid's records from outside the step kernels for many robots at once (a
// mode change, a latch), so that those see - and zero - plain records.  Not in front of a model reset or a copy: that would take
// every steady robot out of its hot rows for nbuf steps to serve a handful.
CDPR_DEV void flush_hot_robot(const GenRecords& v, int nbuf, uint32_t r) {
  const size_t rs = v.plat.stride;
  uint32_t* const c = reinterpret_cast<uint32_t*>(v.rec) + ((size_t)v.lay.slots() * 4 + (size_t)v.lay.rows()) * rs + r;
  const uint32_t step1 = c[0];
  if (step1 == 0u) return;
  const uint32_t mask = c[rs];
  const int step = (int)step1 - 1;
  const uint32_t meta = kGmWasLast | ((uint32_t)nbuf << kGmCountShift) | ((uint32_t)(step % nbuf) << kGmHeadShift) | (kGmField << kGmRunShift);
  float4* const slots = reinterpret_cast<float4*>(v.rec);
  for (int i = 0; i < v.lay.n; ++i) {
    const float ierr = __uint_as_float(c[(size_t)(2 + i) * rs]);
    slots[(size_t)(v.lay.block_a((int)((mask >> i) & 1u), i) + v.lay.nv()) * rs + r] = make_float4(__uint_as_float(meta), __int_as_float(step), ierr, 0.f);
  }
  c[0] = 0u;
}

// ------------------------------------------------------------------------------------------------------------------- model reset

// JointForceCalculator::reset() (JFC.h:69-73) plus the state Load leaves (PLG.cpp:153-157: Position mode, target 0) for the robots
// of the mask; the world clock, the other robots and every pending command stay as they are; the robot's episode clock restarts.
struct ResetWhere {
  const uint8_t* mask;  // uint8[B]
  const float* pose;    // float[B][7], or nullptr = home
  const float* twist;   // float[B][6], or nullptr = zero
  float home[7];        // cdpr_config_t.home_pose (fp32 handles; precision = 64: F64Records::home)
  uint32_t step;        // low word of cdpr_step_count at the call
};

// the robot's pose and twist: its rows of the caller's buffers, or home and zero
CDPR_DEV void reset_rows(const ResetWhere& w, uint32_t r, float (&p)[7], float (&t)[6]) {
#pragma unroll
  for (int c = 0; c < 7; ++c) p[c] = w.pose ? w.pose[(size_t)r * 7 + c] : w.home[c];
#pragma unroll
  for (int c = 0; c < 6; ++c) t[c] = w.twist ? w.twist[(size_t)r * 6 + c] : 0.f;
}

// platform slots 0-3 (+ 4 with FK: the seed follows the pose, as cdpr_set_platform_state has it), the observable image before the
// first publish (the pose, zeros elsewhere: joint rows, twist, FK residual and iterations, flags), the `pid` debug row
CDPR_DEV void reset_platform(const PlatRows& a, uint32_t r, const float (&p)[7], const float (&t)[6]) {
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

CDPR_DEV void model_reset(const ResetWhere& w, const FastRecords& v, uint32_t r) {
  float p[7], t[6];
  reset_rows(w, r, p, t);
  reset_platform(v.plat, r, p, t);
  pid_reset(v, r);
  v.meta[r] = (uint8_t)kMetaPosition;  // call count 0
  for (uint32_t i = 0; i < v.n; ++i) v.target[(size_t)r * v.n + i] = 0.f;
  v.episode_start[r] = w.step;
}

// The whole column of regions A and B (mLastPosition and both Pids of every cable) and the robot's own hot-row word (region C, row
// 0: the stale H slots it stood for have just been zeroed, so nothing is flushed; the robots around it keep their hot rows).
CDPR_DEV void model_reset(const ResetWhere& w, const GenRecords& v, uint32_t r) {
  float p[7], t[6];
  reset_rows(w, r, p, t);
  reset_platform(v.plat, r, p, t);
  const size_t rs = v.plat.stride;
  float4* const sa = reinterpret_cast<float4*>(v.rec) + r;
  for (int sl = 0; sl < v.lay.slots(); ++sl) sa[(size_t)sl * rs] = make_float4(0.f, 0.f, 0.f, 0.f);
  float* const rb = v.rec + (size_t)v.lay.slots() * rs * 4 + r;
  for (int row = 0; row < v.lay.rows(); ++row) rb[(size_t)row * rs] = 0.f;
  rb[(size_t)v.lay.rows() * rs] = 0.f;  // region C, row 0: the robot's hot-row word (a store of its own: folded into the loop above, the
                                        // loop's trip count rows() + 1 goes into a vector counter and a reset of one lane pays 1.8 us more)
  v.mode[r] = (uint8_t)kMetaPosition;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (uint32_t i = 0; i < v.n; ++i) v.latched[k][(size_t)r * v.n + i] = 0.f;
  v.episode_start[r] = w.step;
}

// The double rows of pose, twist and FK estimate (a float pose becomes a double exactly), the image and the `pid` row in double; on
// HOLD handles every cable's mLastPosition row (the one in front of its two Pids) with both Pids.
CDPR_DEV void model_reset(const ResetWhere& w, const F64Records& v, uint32_t r) {
  float p[7], t[6];
  reset_rows(w, r, p, t);
  const size_t st = v.stride;
  double* const S = v.state + r;
  double* const O = v.obs + r;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const double pc = w.pose ? (double)p[c] : v.home[c];
    S[(size_t)(kF64Pose + c) * st] = pc;
    S[(size_t)(kF64StateFk + c) * st] = pc;
    O[(size_t)(kF64Pose + c) * st] = pc;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) S[(size_t)(kF64Twist + c) * st] = (double)t[c];
  for (uint32_t row = kF64Twist; row < v.obs_rows; ++row) O[(size_t)row * st] = 0.0;
  if (v.hold) {
    for (uint32_t i = 0; i < v.n; ++i) S[(size_t)(f64_hold_row((int)v.n, (int)i, 0, (int)v.hold_win) - 1) * st] = 0.0;
    pid_reset(v, r, 1);
  }
  pid_reset(v, r, 0);
  v.meta[r] = (uint8_t)kMetaPosition;
  for (uint32_t i = 0; i < v.n; ++i) v.target[(size_t)r * v.n + i] = 0.f;
  if (v.dbg)
    for (int c = 0; c < CDPR_PID_DEBUG_AXES; ++c) v.dbg[(size_t)r * CDPR_PID_DEBUG_AXES + c] = 0.0;
  v.episode_start[r] = w.step;
}

// -------------------------------------------------------------------------------------------------------------------------- copy

// Robot r with 0 <= source[r] < B, source[r] != r takes over everything robot-indexed the handle owns of robot s = source[r]; every
// other robot is neither read (but as a source) nor written.  A source is itself untouched (source[s] < 0 or source[s] == s), so
// sources are only read and destinations only written: one launch, no scratch copy, no hazard.  The world step is the same for
// both, so nothing is rebased - the rings that follow the world step, the stamps and the `step + 1` hot word are bits moved.
// Every store is row * stride + r, every load row * stride + s.  The loads of a column go out kCopyBatch at a time in front of their
// stores: a lone destination in its wave pays one round trip per batch, not one per row.
constexpr int kCopyBatch = 8;  // independent loads in flight per destination
// a float4 slot as the bits it holds (packed words included): a native vector, which a batch keeps in registers (an array of HIP's
// float4 cost 144 B of scratch)
using CopySlot = uint32_t __attribute__((ext_vector_type(4)));

struct CopyWho {
  const int32_t* source;    // int32[B]
  uint32_t* status;         // uint32[2] = [copied, skipped], zeroed on the stream in front of the launch; or nullptr
};

// The thread's verdict: true for a destination with a valid source `s`.  A destination whose source is out of range or is itself a
// destination is skipped and counted in status[1].  Every lane of the wave comes through here (wave_count_add).
CDPR_DEV bool copy_verdict(const CopyWho& w, uint32_t batch, uint32_t r, uint32_t& s) {
  const int32_t v = r < batch ? w.source[r] : -1;
  const bool wants = v >= 0 && (uint32_t)v != r;
  bool ok = wants && (uint32_t)v < batch;
  if (ok) {
    const int32_t up = w.source[v];
    ok = up < 0 || up == v;
  }
  s = ok ? (uint32_t)v : r;
  if (w.status) {  // (wave-uniform)
    wave_count_add(w.status, ok);
    wave_count_add(w.status + 1, wants && !ok);
  }
  return ok;
}

// rows [0, rows) of a column-per-robot buffer: base[row * stride + r] = base[row * stride + s]
template <typename T>
CDPR_DEV void copy_column(T* base, size_t stride, uint32_t rows, uint32_t r, uint32_t s) {
  const T* const src = base + s;
  T* const dst = base + r;
  uint32_t row = 0;
  for (; row + kCopyBatch <= rows; row += kCopyBatch) {
    T v[kCopyBatch];
#pragma unroll
    for (int j = 0; j < kCopyBatch; ++j) v[j] = src[(size_t)(row + j) * stride];
#pragma unroll
    for (int j = 0; j < kCopyBatch; ++j) dst[(size_t)(row + j) * stride] = v[j];
  }
  for (; row < rows; ++row) dst[(size_t)row * stride] = src[(size_t)row * stride];
}

// a robot-major row: base[r * width + c] = base[s * width + c] (the active target, the latched commands, the `pid` debug row)
template <typename T>
CDPR_DEV void copy_row(T* base, uint32_t width, uint32_t r, uint32_t s) {
  if (!base) return;
  for (uint32_t c = 0; c < width; ++c) base[(size_t)r * width + c] = base[(size_t)s * width + c];
}

// fp32 handles, both paths: every state slot row, the image, the `pid` row
CDPR_DEV void copy_platform(const PlatRows& a, uint32_t r, uint32_t s) {
  copy_column(reinterpret_cast<CopySlot*>(a.state), a.stride, a.n_state, r, s);
  copy_column(reinterpret_cast<CopySlot*>(a.obs), a.stride, a.n_obs, r, s);
  copy_row(a.dbg, CDPR_PID_DEBUG_AXES, r, s);
}

CDPR_DEV void take_over(const FastRecords& v, uint32_t r, uint32_t s) {
  copy_platform(v.plat, r, s);
  v.meta[r] = v.meta[s];
  copy_row(v.target, v.n, r, s);
  v.episode_start[r] = v.episode_start[s];
}

// ... region A, region B and EVERY region C row: the hot-row word travels with the stale H slots it stands for, so nothing is
// flushed or restored, and its mask and integral words travel too
CDPR_DEV void take_over(const GenRecords& v, uint32_t r, uint32_t s) {
  copy_platform(v.plat, r, s);
  copy_column(reinterpret_cast<CopySlot*>(v.rec), v.plat.stride, (uint32_t)v.lay.slots(), r, s);
  copy_column(v.rec + (size_t)v.lay.slots() * v.plat.stride * 4, v.plat.stride, (uint32_t)(v.lay.rows() + v.lay.hot_rows()), r, s);
  v.mode[r] = v.mode[s];
#pragma unroll
  for (int k = 0; k < 3; ++k) copy_row(v.latched[k], v.n, r, s);
  v.episode_start[r] = v.episode_start[s];
}

// ... bits moved, never computed with: the double rows go as 64-bit integers
CDPR_DEV void take_over(const F64Records& v, uint32_t r, uint32_t s) {
  copy_column(reinterpret_cast<uint64_t*>(v.state), v.stride, v.state_rows, r, s);
  copy_column(reinterpret_cast<uint64_t*>(v.obs), v.stride, v.obs_rows, r, s);
  copy_row(reinterpret_cast<uint64_t*>(v.dbg), CDPR_PID_DEBUG_AXES, r, s);
  v.meta[r] = v.meta[s];
  copy_row(v.target, v.n, r, s);
  v.episode_start[r] = v.episode_start[s];
}

}  // namespace cdpr
