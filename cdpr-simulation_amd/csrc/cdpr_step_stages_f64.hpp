// cdpr_step_stages_f64.hpp — stages of one world step of the fp64 kernels as one device function each.
//
// Included by cdpr_step_kernel_f64.hpp behind its helpers (Rot64, ik_row64, chol_*64, the hold functions), not on its own.
// Both kernels call every stage here - cdpr_step_kernel_f64 in all its instantiations (RING_LDS, JCACHE, PR, HOLD, TSTOP, W = 31,
// HW = 32), cdpr_split_kernel_f64 in its cached, LEAN and HOLD builds:
//   joint_coords64      the one-wave kernel's IK stage; the controller wave's two IK stages (hold branch, plain)
//   joint_velocity64    through joint_coords64; the joint-stop sweep of the TSTOP instantiations (qdn)
//   setforce_limits64   the one-wave kernel behind the tension distribution; the controller wave behind the second barrier
//   write_pid_topic64   the one-wave kernel; the controller wave
//   wrench_add64        the world step's loop over the cables in both
//   pose_integrate64    the pose half of the world step in both
// A stage is called only where the call leaves every kernel's scratch, spilled VGPRs, LDS and occupancy as they were and no kernel's
// vector instruction count more than 1 % up (profiles/r16_f64_stages_isa.txt; scripts/isa_compare.py makes the table).  The
// one-wave kernels with hundreds of spilled SGPRs (TSTOP, W = 31, HW = 32, one cable) answer any change in the order of their
// values with another spill pattern, and the lane reads and writes of a spill count as vector instructions.
// STILL SPELLED OUT IN BOTH KERNELS, each tried as a function and taken back (the kernel that moved most, its vector
// instructions against the parent's; a fix to one of these goes to cdpr_step_kernel_f64 AND cdpr_split_kernel_f64):
//   plain Pid::update (Pid.cpp:122-191)       alone within 0.4 % everywhere; with the stages above - all five, or any four of them -
//                                             cdpr_step_kernel_f64<1> + 2.6 % and occupancy 2 -> 1, <1, PR> + 3.2 %
//   per-cable HOLD call (JFC.cpp:59-96)       every HOLD = 2 kernel's scratch moved (20 -> 0 B ... 0 -> 36 B), <3, PR, HOLD = 2> + 4.4 %
//   Newton iterations                         <6, TSTOP> + 4.2 %, worst + 8.5 %; scratch 0 -> 36 B in <7, PR, HOLD = 2, TSTOP>
//   tension of one cable                      <1, W = 31, TSTOP> + 4.9 %; scratch 0 -> 36 B in <1, PR, HOLD = 2, TSTOP>
//   platform part of the observable image     <1, RING_LDS> + 2.4 %, <7, PR, HOLD = 2, TSTOP, HW = 32> + 1.4 %, <7, W = 31> + 1.1 %
//   rigid-body twist update                   <3, PR, HOLD = 2> + 6.4 % and scratch 36 -> 0 B, <8, TSTOP> + 2.1 %
//   lumped legs, joint-stop sweep (one-wave kernel only; tried as lumped_twist64 / travel_stop_sweep64)
//                                             <8, TSTOP> + 2.1 %, <1, TSTOP> + 4.8 %
// Everything is forced inline and written with explicit fma (-ffp-contract=off): same statements, same order, same bits.
// Rules for a new stage: what it READS goes in by value, as scalars - the F64Args fields, and the caller's long-lived registers
// too (the platform's v and om as six doubles: the same stage taking `const double (&v)[3]` moved twenty TSTOP kernels by 1 - 5 %);
// what it WRITES goes through references to the caller's arrays; short-lived locals (a structure-matrix row, the wrench) may be
// references either way.
#pragma once

namespace cdpr {

// Joint::GetVelocity of a prismatic joint restated: qdot = -J [v; w] with the cable's row of the structure matrix
__device__ __forceinline__ double joint_velocity64(const double (&j)[6], double vx, double vy, double vz, double wx, double wy, double wz) {
  return -fma(j[5], wz, fma(j[4], wy, fma(j[3], wx, fma(j[2], vz, fma(j[1], vy, j[0] * vx)))));
}
// ... and Joint::Position: q = L0 - L
__device__ __forceinline__ void joint_coords64(double l0, double L, const double (&j)[6], double vx, double vy, double vz, double wx, double wy, double wz, double& q, double& qd) {
  q = l0 - L;
  qd = joint_velocity64(j, vx, vy, vz, wx, wy, wz);
}

// Joint::SetForce limits of cable i: the velocity truncation ([EXT]: no pushing a runaway joint further out), then the effort clamp
// (cube.sdf:438); and the cable's travel-limit flag
__device__ __forceinline__ double setforce_limits64(double applied, double q, double qd, double vel_limit, double effort, int travel_on, double travel_lo, double travel_hi, int i,
                                                    uint32_t& lim) {
  if (vel_limit > 0.0) applied = ((qd > vel_limit && applied > 0.0) || (qd < -vel_limit && applied < 0.0)) ? 0.0 : applied;
  if (effort >= 0.0) applied = fmax(fmin(applied, effort), -effort);
  if (travel_on && (q < travel_lo || q > travel_hi)) lim |= 1u << i;
  return applied;
}

// `pid` topic of one robot (d = its double[9] record), cable 0 only (PLG.cpp:223-227; Pid.cpp:139-142,158-168): stale entries
// stay where the Pid did not run this step
__device__ __forceinline__ void write_pid_topic64(double* d, bool ran, double p, double i, double dd, double des, double applied0) {
  if (ran) {
    d[0] = p;
    d[1] = i;
    d[2] = dd;
    d[3] = des;
  }
  d[4] = applied0;
}

// One cable's share of the wrench: w -= J^T (applied - d qdot), a unilateral cable does not push
__device__ __forceinline__ void wrench_add64(const double (&j)[6], double damping, int unilateral, double qd, double applied, double (&w)[6]) {
  double t = fma(-damping, qd, applied);
  if (unilateral) t = fmax(t, 0.0);
#pragma unroll
  for (int c = 0; c < 6; ++c) w[c] = fma(-j[c], t, w[c]);
}

// Pose half: p += dt v, q += dt / 2 (0, om) (x) q, renormalised
__device__ __forceinline__ void pose_integrate64(double dt, double half_dt, double vx, double vy, double vz, double wx, double wy, double wz, double (&p)[3], double (&q4)[4]) {
  p[0] = fma(dt, vx, p[0]);
  p[1] = fma(dt, vy, p[1]);
  p[2] = fma(dt, vz, p[2]);
  const double h = half_dt, x = q4[0], y = q4[1], z = q4[2], ww = q4[3];
  const double nx = fma(h, fma(-wz, y, fma(wy, z, ww * wx)), x);
  const double ny = fma(h, fma(-wx, z, fma(wz, x, ww * wy)), y);
  const double nz = fma(h, fma(-wy, x, fma(wx, y, ww * wz)), z);
  const double nw = fma(-h, fma(wz, z, fma(wy, y, wx * x)), ww);
  const double inv = rsqrt64(fma(nw, nw, fma(nz, nz, fma(ny, ny, nx * nx))));
  q4[0] = nx * inv;
  q4[1] = ny * inv;
  q4[2] = nz * inv;
  q4[3] = nw * inv;
}

}  // namespace cdpr
