// cdpr_done.hpp — the verdict of a done rule (cdpr_evaluate_done[_device], cdpr_reset_done_device): which robots of the batch a loop
// should put back, and why.  A pure function of what the getters would return at that point of the stream: the current pose and
// twist (platform rows of the state), the FK residual, the tension-distribution flag and the travel-limit bits of the last
// published step (they travel with the observables), the robot's episode start (the world step of its last model reset) and the
// world-step counter.  Two kernels, one per platform layout: the float4 slot rows of the fp32 handles (both controller paths keep
// the platform in slots 0-3 and the flags in observable slot 3) and the double rows of the precision = 64 handles.  No controller
// record is read, so hot rows, record layouts and the cable count do not matter here.
//
// As the latch, reset and copy kernels (cdpr_robot_records.hpp): one thread per robot, 256 per block, every load row * stride + r
// (a wave reads whole rows: 80 B per robot in float, 136 B in double, 4 B of episode start), no LDS, no scratch.  Straight-line: a
// test the rule leaves disabled is computed and masked out by the wave-uniform `enable` word; the lanes past the batch read robot
// B - 1 and contribute nothing.  Counts: one ballot and one popcount per enabled reason, lane 0 of each wave adds the non-zero ones
// to global memory with an ordinary atomicAdd.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_kernels.hpp"

namespace cdpr {

// what a robot's verdict is computed from, in the precision of the handle
template <typename T>
struct DoneInputs {
  T p[7];             // x y z qx qy qz qw
  T t[6];             // linear, angular
  T fk_residual;
  uint32_t flags;     // pack_flags: bit 0 tension distribution infeasible, bit 1 + i cable i outside its travel limits
  uint32_t age;       // world steps since the robot's last model reset (wraps with the low word of the step counter)
};

CDPR_DEV float done_fma(float a, float b, float c) { return fmaf(a, b, c); }
CDPR_DEV double done_fma(double a, double b, double c) { return fma(a, b, c); }
CDPR_DEV bool done_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }            // false for NaN and +-inf
CDPR_DEV bool done_finite(double x) { return fabs(x) <= 1.7976931348623157e+308; }

// The reason word: the OR of the rule's enabled bits whose condition holds.  Every comparison is an ordinary one (false on NaN);
// only NONFINITE reports a NaN.  The rule's floats are promoted to T.
template <typename T>
CDPR_DEV uint32_t done_reason(const cdpr_done_rule_t& k, const DoneInputs<T>& s) {
  bool bad = false, out = false;
#pragma unroll
  for (int c = 0; c < 7; ++c) bad = bad || !done_finite(s.p[c]);
#pragma unroll
  for (int c = 0; c < 6; ++c) bad = bad || !done_finite(s.t[c]);
#pragma unroll
  for (int c = 0; c < 3; ++c) out = out || s.p[c] < (T)k.pos_lo[c] || s.p[c] > (T)k.pos_hi[c];
  // R33 = 1 - 2 (qx^2 + qy^2) / (q . q): the platform's up axis on the world's (no normalisation of the pose is assumed)
  const T tilt = done_fma(s.p[3], s.p[3], s.p[4] * s.p[4]);
  const T qq = done_fma(s.p[6], s.p[6], done_fma(s.p[5], s.p[5], tilt));
  const T r33 = (T)1 - ((T)2 * tilt) / qq;
  const T vv = done_fma(s.t[2], s.t[2], done_fma(s.t[1], s.t[1], s.t[0] * s.t[0]));
  const T ww = done_fma(s.t[5], s.t[5], done_fma(s.t[4], s.t[4], s.t[3] * s.t[3]));
  const T max_speed = (T)k.max_speed, max_rate = (T)k.max_rate;
  uint32_t r = 0u;
  r |= bad ? CDPR_DONE_NONFINITE : 0u;
  r |= out ? CDPR_DONE_WORKSPACE : 0u;
  r |= r33 < (T)k.min_up ? CDPR_DONE_TILT : 0u;
  r |= vv > max_speed * max_speed ? CDPR_DONE_SPEED : 0u;
  r |= ww > max_rate * max_rate ? CDPR_DONE_RATE : 0u;
  r |= s.fk_residual > (T)k.max_fk_residual ? CDPR_DONE_FK_RESIDUAL : 0u;
  r |= (s.flags & 1u) ? CDPR_DONE_INFEASIBLE : 0u;
  r |= (s.flags >> 1) ? CDPR_DONE_TRAVEL : 0u;
  r |= s.age >= k.max_steps ? CDPR_DONE_TIMEOUT : 0u;
  return r & k.enable;
}

struct DoneOut {
  uint8_t* mask;        // uint8[B]: exactly 0 or 1
  uint32_t* reason;     // uint32[B], or nullptr
  uint32_t* counts;     // uint32[CDPR_DONE_COUNTS], zeroed on the stream in front of the launch, or nullptr
};

// rows [0, B) of the caller's buffers and the wave's share of the counts; `live`: the lane has a robot
CDPR_DEV void done_store(const DoneOut& o, uint32_t enable, uint32_t r, bool live, uint32_t reason) {
  reason = live ? reason : 0u;
  if (live) {
    o.mask[r] = reason ? (uint8_t)1 : (uint8_t)0;
    if (o.reason) o.reason[r] = reason;
  }
  if (!o.counts) return;  // (wave-uniform, as `enable` below)
  if (!wave_count_add(o.counts, reason != 0u)) return;
  for (uint32_t k = 0; k + 1u < (uint32_t)CDPR_DONE_COUNTS; ++k)
    if ((enable >> k) & 1u) wave_count_add(o.counts + 1u + k, (reason >> k) & 1u);
}

#ifndef CDPR_DONE_NO_KERNELS  // (cdpr_env.hpp takes done_reason and done_store and leaves the two kernels to cdpr_engine_done.hip)
// fp32 handles, both controller paths: state slots 0-3 = [x y z qx | qy qz qw vx | vy vz wx wy | wz ...], observable slot 3 =
// [wz | fk residual | fk iterations | flags] of the last published step
struct DoneArgs {
  cdpr_done_rule_t rule;
  const float4* state;
  const float4* obs;
  const uint32_t* episode_start;  // uint32[B]
  size_t stride;
  uint32_t batch;
  uint32_t step;                  // low word of the world-step counter at the call
  DoneOut out;
};

static __global__ __launch_bounds__(256) void cdpr_done_kernel(const DoneArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const bool live = r < a.batch;
  const uint32_t c = live ? r : a.batch - 1u;
  const size_t st = a.stride;
  const float4 s0 = a.state[0 * st + c], s1 = a.state[1 * st + c], s2 = a.state[2 * st + c], s3 = a.state[3 * st + c];
  const float4 o3 = a.obs[3 * st + c];
  DoneInputs<float> s;
  s.p[0] = s0.x, s.p[1] = s0.y, s.p[2] = s0.z, s.p[3] = s0.w, s.p[4] = s1.x, s.p[5] = s1.y, s.p[6] = s1.z;
  s.t[0] = s1.w, s.t[1] = s2.x, s.t[2] = s2.y, s.t[3] = s2.z, s.t[4] = s2.w, s.t[5] = s3.x;
  s.fk_residual = o3.y;
  s.flags = (uint32_t)(int)o3.w;  // (as cdpr_get_td_state / cdpr_get_limit_state read the component)
  s.age = a.step - a.episode_start[c];
  done_store(a.out, a.rule.enable, r, live, done_reason(a.rule, s));
}

// precision = 64 handles: state rows kF64Pose + 0..6 and kF64Twist + 0..5, observable rows kF64ObsResidual and kF64ObsFlags
struct DoneF64Args {
  cdpr_done_rule_t rule;
  const double* state;
  const double* obs;
  const uint32_t* episode_start;
  size_t stride;
  uint32_t batch;
  uint32_t step;
  DoneOut out;
};

static __global__ __launch_bounds__(256) void cdpr_done_f64_kernel(const DoneF64Args a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const bool live = r < a.batch;
  const uint32_t c = live ? r : a.batch - 1u;
  const size_t st = a.stride;
  const double* const S = a.state + c;
  const double* const O = a.obs + c;
  DoneInputs<double> s;
#pragma unroll
  for (int i = 0; i < 7; ++i) s.p[i] = S[(size_t)(kF64Pose + i) * st];
#pragma unroll
  for (int i = 0; i < 6; ++i) s.t[i] = S[(size_t)(kF64Twist + i) * st];
  // (the residual has no double getter: it is taken as cdpr_get_fk_state hands it out, rounded to float, so that the verdict stays
  // a function of the getters' outputs)
  s.fk_residual = (double)(float)O[(size_t)kF64ObsResidual * st];
  s.flags = (uint32_t)(int32_t)O[(size_t)kF64ObsFlags * st];  // (as the flags getters read the row)
  s.age = a.step - a.episode_start[c];
  done_store(a.out, a.rule.enable, r, live, done_reason(a.rule, s));
}
#endif  // CDPR_DONE_NO_KERNELS

}  // namespace cdpr
