// cdpr_step_stages.hpp — stages of one world step of the fp32 kernels as one device function each.
//
// Included by cdpr_step_kernel.hpp behind its helpers (ik_pairs, jt_times, normal_solve, Platform), not on its own.
// Callers today:
//   unpack_platform   cdpr_step_kernel, cdpr_onestep_kernel, split_controller_wave, cdpr_gen_step_kernel, cdpr_gen_split_kernel,
//                     cdpr_gen_lean_kernel and its cold tail, cdpr_step_kernel_pair
//   write_pid_topic   the same but the lean kernel and its cold tail (lean_controller_epilogue writes the same five words with
//                     stores predicated through their offsets: it must not contain a divergent branch)
//   setforce_limits   cdpr_onestep_kernel, split_controller_wave, cdpr_gen_split_kernel, lean_controller_epilogue, cdpr_step_kernel_pair
//   joint_coords      cdpr_step_kernel_pair, cdpr_pair_stream_kernel
//   newton_fk         cdpr_solver_kernel's FK branch
// Every other kernel still spells these statements out (cdpr_step_kernel and cdpr_gen_step_kernel the limits; the
// lane-per-robot kernels the joint coordinates and the Newton loop): a fix to one of them goes to the function here AND to
// those kernels.  A stage is called only where the call leaves every kernel's registers, spills, scratch, LDS and
// occupancy as they were (profiles/r08_stage_factoring_isa.txt; scripts/isa_compare.py makes the table).
// Everything is forced inline and written with explicit fma (-ffp-contract=off): same statements, same order, same bits.
// Rules for a new stage: take a Platform by value, not by reference; take the StepArgs scalars it reads in a loop as scalars.
#pragma once

namespace cdpr {

// Platform rows 0..2 and the first word of row 3 -> Platform (state slots: see the top of cdpr_step_kernel.hpp).
template <typename V4>
CDPR_DEV void unpack_platform(const V4& p0, const V4& p1, const V4& p2, float wz, Platform& s) {
  s.px = p0.x; s.py = p0.y; s.pz = p0.z; s.qx = p0.w;
  s.qy = p1.x; s.qz = p1.y; s.qw = p1.z; s.vx = p1.w;
  s.vy = p2.x; s.vz = p2.y; s.wx = p2.z; s.wy = p2.w;
  s.wz = wz;
}

// Joint coordinates of the prismatic joints from the IK rows (Joint::Position / GetVelocity restated): q = L0 - L,
// qdot = -J [v; w].
template <int NP>
CDPR_DEV void joint_coords(const Platform s, const v2f (&len)[NP], const v2f (&l0)[NP], const v2f (&jac)[NP][6], v2f (&q)[NP], v2f (&qd)[NP]) {
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    q[k] = l0[k] - len[k];
    qd[k] = -fma2(s.wz, jac[k][5], fma2(s.wy, jac[k][4], fma2(s.wx, jac[k][3],
                  fma2(s.vz, jac[k][2], fma2(s.vy, jac[k][1], splat(s.vx) * jac[k][0])))));
  }
}

// Newton-Raphson forward kinematics ([NEW] SURVEY 8(a) row 14): the pose estimate (x, y, z, quaternion) is moved until the
// cable lengths it implies meet the measured ones `len`, at most `iters` damped Gauss-Newton steps ((J^T J + lambda I) d =
// J^T r); a lane whose residual has fallen below `tol` stops moving (and counting) but keeps executing.  Leaves the
// structure matrix AT THE FINAL ESTIMATE in jest (the tension distribution's) and the closing residual max |L* - L(est)|.
// The step kernels restate this loop (each with its own pins: LOWREG's opaque geometry offset per iteration, the
// estimator wave's per-iteration stamps); the statements and their order are these.
template <int N>
CDPR_DEV void newton_fk(int iters, float lambda, float tol, const float* geo, const v2f (&len)[cable_pairs(N)], float& x, float& y, float& z, float& qx,
                        float& qy, float& qz, float& qw, v2f (&jest)[cable_pairs(N)][6], float& fk_res, int& fk_it) {
  constexpr int NP = cable_pairs(N);
  v2f elen[NP], unused[NP];
  bool active = true;
  for (int it = 0; it < iters; ++it) {
    ik_pairs<N, false>(geo, x, y, z, qx, qy, qz, qw, elen, jest, unused);
    v2f res[NP];
    v2f rm = splat(0.f);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      res[k] = len[k] - elen[k];
      rm = max2(rm, abs2(res[k]));
    }
    active = active && !(fmaxf(rm.x, rm.y) < tol);
    float g[6];
    jt_times<NP>(jest, res, g);
    normal_solve<NP>(jest, lambda, g);
    if (active) {
      x += g[0];
      y += g[1];
      z += g[2];
      quat_apply_rotvec(qx, qy, qz, qw, g[3], g[4], g[5]);
      ++fk_it;
    }
  }
  ik_pairs<N, false>(geo, x, y, z, qx, qy, qz, qw, elen, jest, unused);
  v2f rm = splat(0.f);
#pragma unroll
  for (int k = 0; k < NP; ++k) rm = max2(rm, abs2(len[k] - elen[k]));
  fk_res = fmaxf(rm.x, rm.y);
}

// Joint::SetForce limits: the velocity truncation ([EXT]: no pushing a runaway joint further out), then the effort clamp
// (cube.sdf:438).
template <int NP>
CDPR_DEV void setforce_limits(const StepArgs& a, const v2f (&qd)[NP], v2f (&applied)[NP]) {
  if (a.vel_limit > 0.f) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      applied[k].x = (qd[k].x > a.vel_limit && applied[k].x > 0.f) || (qd[k].x < -a.vel_limit && applied[k].x < 0.f) ? 0.f : applied[k].x;
      applied[k].y = (qd[k].y > a.vel_limit && applied[k].y > 0.f) || (qd[k].y < -a.vel_limit && applied[k].y < 0.f) ? 0.f : applied[k].y;
    }
  }
  if (a.effort >= 0.f) {
#pragma unroll
    for (int k = 0; k < NP; ++k) applied[k] = max2(min2(applied[k], splat(a.effort)), splat(-a.effort));
  }
}

// `pid` topic of one robot (d = its float[9] record), cable 0 only (PLG.cpp:223-227; Pid.cpp:139-142,158-168): stale
// entries stay where a term was not computed this step.  pi: the proportional and integral terms (and the target) are
// this step's; dw: the derivative term is.  The first-generation Pid computes all or none (pi == dw).
CDPR_DEV void write_pid_topic(float* d, bool pi, bool dw, float p, float i, float dd, float des, float applied0) {
  if (pi) {
    d[0] = p;
    d[1] = i;
    d[3] = des;
  }
  if (dw) d[2] = dd;
  d[4] = applied0;
}

}  // namespace cdpr
