// cdpr_onestep_kernel.hpp — the one-world-step-per-launch kernel (gfx950, fp32, lane-per-robot), second generation.
//
// Same arithmetic as cdpr_step_kernel<N, FK, TD, SINGLE = true> (the device functions are shared: the leaf helpers of
// cdpr_step_kernel.hpp and the stages of cdpr_step_stages.hpp that this file calls - unpack_platform, setforce_limits,
// write_pid_topic; the other stages are restated statement by statement, with a pointer where a shared function exists -
// and the file is compiled with -ffp-contract=off, so the two are bit-identical — tested), re-staged around what the
// profile of the first generation showed (profiles/r02a_onestep_summary.json: one wave per SIMD, 47 % of wave cycles issuing,
// 27 % waiting on memory, 25 % dependent-issue stalls):
//
//   * the controller rows (20 ring rows + 2 integral rows at n = 8: 22 of the 29 rows a robot reads) are NOT needed
//     until the per-cable PID, but as ordinary loads they either stall the wave right away or sit in 88 VGPRs while
//     the Newton stage wants every register.  They go global -> LDS directly (global_load_lds_dwordx4: one 1 KiB
//     row per wave-instruction, lane-linear, no VGPR destination), are issued once the platform rows have arrived,
//     stay in flight under the whole Newton-Raphson stage, and are read back with ds_read_b128 for the PID;
//   * the stage order is IK -> early observables -> Newton FK -> [wait for the DMA] PID -> TD -> world step, so the
//     only memory wait on the critical path is the first round trip of the 5 platform rows;
//   * the observables that are final after the IK (pose, twist, joint position, joint velocity: 7 of 10 rows) are
//     stored before the Newton stage: the stores drain under compute instead of forming a tail;
//   * nothing of the true-state IK but the measured lengths L* lives through the Newton stage: the structure
//     matrix is rebuilt afterwards (one more IK evaluation, ~4 % more instructions) instead of holding 64 VGPRs.
//
// LDS per wave: 16 floats x cable pairs of geometry + (controller rows + command rows) x 1 KiB = 24.25 KiB at n = 8;
// 4 waves per CU (one per SIMD) use 97 KiB of the CU's 160 KiB.
#pragma once
#include "cdpr_step_kernel.hpp"

namespace cdpr {

// One controller / command row of the calling wave, global -> LDS without a register destination: lane l copies the
// 16 bytes at src to dst_row + 16 l (the LDS side of an LDS-DMA is always wave-base + lane * size).
CDPR_DEV void row_to_lds(const float4* src, float4* dst_row) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst_row, 16, 0, 0);
}

// Row stores go through store_slot (one buffer descriptor per row).  One descriptor per BUFFER with the row as the scalar
// offset operand was measured too: 100 fewer scalar instructions and 14 -> 6 spilled SGPRs, the same time within noise
// (profiles/r02f_onestep_v2_variants_ab.txt) - and the FK instantiations at n = 8 then failed the bit-identity and
// parity tests on MI355X (cause not found in the ISA), so that form is not in the tree.  Also measured, neither faster:
// weights staged in LDS instead of kernel arguments, cable constants re-read per Newton iteration.

// Pid::update for every cable pair (Pid.cpp:122-191; the same statements as in cdpr_step_kernel).  PR (per-robot handles):
// `calls` and `is_vel` are the lane's own, the coefficients and weights are selected per lane, and a robot whose Pid was
// just reset (calls == 0: "first call returns 0", Pid.cpp:123-126) keeps force 0 and its integral.
// FULL: the caller knows that the derivative window holds nbuf samples (calls >= nbuf).
template <int NP, bool PR = false, bool FULL = false>
CDPR_DEV void pid_pairs(const StepArgs& a, int calls, bool is_vel, const v2f (&desired)[NP], const v2f (&actual)[NP], const v2f (&win)[NP][kWin],
                        v2f (&ierr)[NP], v2f (&f)[NP], v2f (&e_new)[NP], float& dbg_p, float& dbg_i, float& dbg_d, bool is_force = false) {
  const PidCoef c = pid_coef<PR>(a, is_vel);
  const bool run = (!PR || calls != 0) && !is_force;  // is_force (PR only): the robot is driven open loop (JFC.cpp:67-70)
  const bool full = FULL || calls >= c.nbuf;  // derive(): 0 until the window holds nbuf samples (Pid.cpp:200-203)
  // the host put the weights of this launch's ring position (StepArgs::ring_slot) into the arguments; on per-robot handles
  // both Pids fit the same window (same length and degree: cdpr_create sends anything else down the general path), so
  // the weights stay scalars whatever the lane's mode
  const float (&wt)[kWin + 2] = a.wrow;
  v2f error[NP], acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    error[k] = desired[k] - actual[k];
    acc[k] = splat(wt[kWin]) * error[k];
  }
#pragma unroll
  for (int j = 0; j < kWin; ++j) {
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = fma2(wt[j], win[k][j], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const v2f p_term = splat(c.kp) * error[k];
    const v2f prev_ierr = ierr[k];
    v2f ie = fma2(a.dt, error[k], prev_ierr);
    const v2f i_term = splat(c.ki) * ie;
    const v2f i_cl = max2(min2(i_term, splat(c.imax)), splat(c.imin));  // Pid.cpp:143-152
    const v2f ie_cl = i_cl * splat(c.inv_ki);
    ie.x = (i_cl.x != i_term.x) ? ie_cl.x : ie.x;
    ie.y = (i_cl.y != i_term.y) ? ie_cl.y : ie.y;
    const v2f derived = full ? acc[k] * splat(a.inv_dt) : splat(0.f);
    const v2f d_term = splat(c.kd) * derived;
    const v2f cmd = fma2(c.kf, desired[k], p_term) + i_cl + d_term;
    v2f out = c.clamp ? max2(min2(cmd, splat(c.cmax)), splat(c.cmin)) : cmd;  // Pid.cpp:175-177
    const v2f bumped = fma2(splat(a.dt) * error[k], splat(c.ki), out);             // Pid.cpp:181-184
    ie.x = (out.x != cmd.x) ? prev_ierr.x : ie.x;
    ie.y = (out.y != cmd.y) ? prev_ierr.y : ie.y;
    out.x = (out.x != cmd.x) ? bumped.x : out.x;
    out.y = (out.y != cmd.y) ? bumped.y : out.y;
    ierr[k] = run ? ie : prev_ierr;
    f[k] = run ? out : (is_force ? desired[k] : splat(0.f));
    e_new[k] = error[k];
    if (k == 0) {
      dbg_p = p_term.x;
      dbg_i = i_term.x;
      dbg_d = d_term.x;
    }
  }
}

// PERSIST (batches beyond one robot per hardware lane): the grid is one wave per SIMD and every wave walks over blocks of
// 64 robots, blockIdx.x, blockIdx.x + gridDim.x, ...  A launch whose waves each take ONE block is bulk-synchronous (load,
// ~8 us of arithmetic, store), and a second wave on the same SIMD runs in phase with the first and adds its whole issue
// time (profiles/r04_cliff_analysis.txt); here the NEXT block's rows are requested while the current block computes -
// its controller rows and Joy by LDS-DMA as soon as the PID stage has read the staged ones, its platform rows into
// registers right after - so from the second block on a wave never waits for memory.
// A row load the compiler does not track (inline asm): the persistent kernel requests the next block's platform rows a
// whole block ahead and waits for them with an explicit vmcnt(N) that leaves the N later operations (the next block's
// LDS-DMA, this block's last observable stores) in flight.  Through ordinary loads the compiler would drain EVERY
// outstanding memory operation at their first use (it does so whenever an LDS-DMA is pending), and the DMA - 24 KiB per
// wave that the next block needs 9 us later - would have to land within 2 us of its issue, all waves at once.
typedef float f32x4 __attribute__((ext_vector_type(4)));
CDPR_DEV f32x4 load_slot_untracked(const float4* base, size_t stride, int slot, uint32_t off) {
  const char* p = reinterpret_cast<const char*>(base + (size_t)slot * stride) + off;
  f32x4 v;
  // (into ACCUMULATION registers: the compiler takes an asm's result for valid at once and may copy it anywhere - a
  //  vector-register result it moved into a spare AGPR straight away, before the data was there; an AGPR result has no
  //  reason to move before its use.  Checked in the ISA: nothing reads these registers between the load and the wait.)
  asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(v) : "v"(p) : "memory");
  return v;
}
// s_waitcnt immediate (gfx9): vmcnt = n (6 bits, split 3:0 | 15:14), expcnt and lgkmcnt untouched
constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

template <int N, bool FK, bool TD, bool PERSIST = false>
__global__ __launch_bounds__(64, 1) void cdpr_onestep_kernel(const StepArgs a_in) {
  const StepArgs& a = a_in;  // (shadowed inside the block loop, see there)
  constexpr int NP = cable_pairs(N);
  constexpr int P = plat_slots(FK);
  constexpr int G = joint_groups(N);
  constexpr int NH = (NP + 1) / 2;           // integral ("hot") rows
  constexpr int kCtrl = 5 * NP + NH;         // controller rows of one robot
  constexpr bool kCmdLds = (N % 4) == 0;     // Joy rows are float4-addressable: stage them through LDS as well
  constexpr int kCmdRows = kCmdLds ? N / 4 : 0;
  __shared__ __attribute__((aligned(16))) float lds[NP * kGeomFloatsPerPair];
  __shared__ float4 stage[kCtrl + (kCmdRows ? kCmdRows : 1)][64];

  const uint32_t lane = threadIdx.x;
  const size_t st0 = a.stride;
  const uint32_t nblocks = (a.batch + 63u) / 64u;
  uint32_t blk = blockIdx.x;
  uint32_t r = blk * 64u + lane;
  uint32_t rr = (r < a.batch) ? r : (a.batch - 1u);  // tail lanes shadow the last robot, stores are masked
  bool live = r < a.batch;
  uint32_t off = rr * 16u, woff = r * 16u;

  // ---- loads that the first stages need: geometry (oldest), platform rows, and the Joy when it is not LDS-staged
  CDPR_STAMP(0);
  const float gval = (lane < NP * kGeomFloatsPerPair) ? a.geom[lane] : 0.f;
  float4 p0 = load_slot(a.state, st0, 0, off), p1 = load_slot(a.state, st0, 1, off), p2 = load_slot(a.state, st0, 2, off),
         p3 = load_slot(a.state, st0, 3, off);
  float4 p4 = make_float4(0.f, 0.f, 0.f, 1.f);
  if (FK) p4 = load_slot(a.state, st0, 4, off);
  if (lane < NP * kGeomFloatsPerPair) lds[lane] = gval;
  const bool force_mode = (a.flags & kFlagForceMode) != 0u;  // UpdateMode::Force (JFC.cpp:67-70): no Pid, no controller rows
  const bool first_world = (a.flags & kFlagFirstWorldStep) != 0u;
  const bool run_pid = !first_world && !force_mode && a.pid_calls != 0;  // wave-uniform (Pid.cpp:123-126: the first call returns 0)
  bool staged = false;  // PERSIST: this block's controller rows were requested during the previous block

  for (;;) {  // (one pass unless PERSIST)
  // (opaque per block: every row address of the loop is loop-invariant, and hoisted out of it they overflow the scalar
  //  register file into v_writelane / v_readlane pairs - measured: 762 of them)
  size_t st = st0;
  uint32_t goff = 0;  // (likewise the geometry in LDS: hoisted, its 7n values would ride through the whole loop in registers)
  if (PERSIST) asm volatile("" : "+s"(st), "+v"(goff));
  const float* const geo = lds + goff;
  // ... and the kernel arguments themselves: every scalar the loop body reads would stay in a register across the whole
  // loop, and everything computed from them once (packed broadcasts, negated constants) with it; read through an opaque
  // pointer to the kernarg segment they are scalar loads of THIS block, as in the one-block kernel
  const StepArgs a = block_args<PERSIST>(a_in);
  v2f desired[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) desired[k] = splat(0.f);
  const float* cp = a.cmd + (size_t)rr * N;  // never null: before the first Joy the latched buffer holds zeros
  if (!kCmdLds || force_mode) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i & 1)
        desired[i / 2].y = cp[i];
      else
        desired[i / 2].x = cp[i];
    }
  }
  // single-wave workgroup: LDS operations of one wave execute in order (see cdpr_step_kernel)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  Platform s;
  unpack_platform(p0, p1, p2, p3.x, s);
  float fkx = p3.y, fky = p3.z, fkz = p3.w, fkqx = p4.x, fkqy = p4.y, fkqz = p4.z, fkqw = p4.w;

  // ---- controller rows and the Joy: global -> LDS, in flight until the PID stage.  Issued AFTER the platform rows
  //      are in registers: hipcc drains every outstanding VMEM operation (vmcnt(0)) at the first use of an ordinary
  //      load's result while an LDS-DMA is pending, so the DMA must not be pending yet when the platform rows are used.
  {
    // every ordinary load issued so far is consumed here (data dependence: no use of one can sink below the DMA issue)
    float keep = (s.px + s.qy) + (s.vy + s.wz) + fkqw;
#pragma unroll
    for (int k = 0; k < NP; ++k) keep += desired[k].x + desired[k].y;
    asm volatile("" ::"v"(keep));
    if (run_pid && !staged) {
#pragma unroll
      for (int j = 0; j < kCtrl; ++j)
        row_to_lds(reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.state + (size_t)(P + j) * st) + off), &stage[j][0]);
      if (kCmdLds) {
#pragma unroll
        for (int g = 0; g < kCmdRows; ++g) row_to_lds(reinterpret_cast<const float4*>(cp) + g, &stage[kCtrl + g][0]);
      }
    }
  }

  // ---- PERSIST: the next block's platform rows, requested a whole block ahead (untracked: see load_slot_untracked)
  const uint32_t nblk = blk + gridDim.x;
  const bool more = PERSIST && nblk < nblocks;
  uint32_t nr = 0, nrr = 0;
  f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = n0, n2 = n0, n3 = n0, n4 = {0.f, 0.f, 0.f, 1.f};
  if (PERSIST && more) {
    nr = nblk * 64u + lane;
    nrr = (nr < a.batch) ? nr : (a.batch - 1u);
    const uint32_t noff = nrr * 16u;
    n0 = load_slot_untracked(a.state, st, 0, noff), n1 = load_slot_untracked(a.state, st, 1, noff);
    n2 = load_slot_untracked(a.state, st, 2, noff), n3 = load_slot_untracked(a.state, st, 3, noff);
    if (FK) n4 = load_slot_untracked(a.state, st, 4, noff);
  }

  CDPR_STAMP(1);
  // ---- IK on the state at t_k: joint positions and rates (observables), measured lengths L* for the estimator
  v2f len[NP], q[NP], qd[NP], jac[NP][6];
  {
    v2f l0[NP];
    ik_pairs<N, true>(geo, s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, len, jac, l0);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      q[k] = l0[k] - len[k];
      qd[k] = -fma2(s.wz, jac[k][5], fma2(s.wy, jac[k][4], fma2(s.wx, jac[k][3],
                    fma2(s.vz, jac[k][2], fma2(s.vy, jac[k][1], splat(s.vx) * jac[k][0])))));
    }
  }
  const bool publish = (a.publish_mask & 1ull) != 0ull;
  if (publish && live) {  // the part of the observables that is final already (PLG.cpp:248-280)
    store_slot(a.obs, st, 0, woff, make_float4(s.px, s.py, s.pz, s.qx));
    store_slot(a.obs, st, 1, woff, make_float4(s.qy, s.qz, s.qw, s.vx));
    store_slot(a.obs, st, 2, woff, make_float4(s.vy, s.vz, s.wx, s.wy));
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k0 = 2 * g, k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
      const bool has = (2 * g + 1 < NP);
      store_slot(a.obs, st, 4 + g, woff, make_float4(q[k0].x, q[k0].y, has ? q[k1].x : 0.f, has ? q[k1].y : 0.f));
      store_slot(a.obs, st, 4 + G + g, woff, make_float4(qd[k0].x, qd[k0].y, has ? qd[k1].x : 0.f, has ? qd[k1].y : 0.f));
    }
  }

  CDPR_STAMP(2);
  // ---- Newton-Raphson forward kinematics ([NEW] SURVEY 8(a) row 14); only len lives in from the true state
  float fk_res = 0.f;
  int fk_it = 0;
  v2f jest[NP][6];
  if (FK) {
    v2f elen[NP], unused[NP];
    bool active = true;
    for (int it = 0; it < a.fk_iters; ++it) {
      ik_pairs<N, false>(geo, fkx, fky, fkz, fkqx, fkqy, fkqz, fkqw, elen, jest, unused);
      v2f res[NP];
      v2f rm = splat(0.f);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        res[k] = len[k] - elen[k];
        rm = max2(rm, abs2(res[k]));
      }
      active = active && !(fmaxf(rm.x, rm.y) < a.fk_tol);
      float g[6];
      jt_times<NP>(jest, res, g);
      normal_solve<NP>(jest, a.fk_lambda, g);
      if (active) {
        fkx += g[0];
        fky += g[1];
        fkz += g[2];
        quat_apply_rotvec(fkqx, fkqy, fkqz, fkqw, g[3], g[4], g[5]);
        ++fk_it;
      }
    }
    ik_pairs<N, false>(geo, fkx, fky, fkz, fkqx, fkqy, fkqz, fkqw, elen, jest, unused);
    v2f rm = splat(0.f);
#pragma unroll
    for (int k = 0; k < NP; ++k) rm = max2(rm, abs2(len[k] - elen[k]));
    fk_res = fmaxf(rm.x, rm.y);
  }

  CDPR_STAMP(3);
  // ---- per-cable force (PLG.cpp:222-228 -> JFC.cpp:59-96 -> Pid.cpp:122-191) on the controller rows from LDS
  v2f f[NP], e_new[NP], ierr[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    f[k] = splat(0.f);
    e_new[k] = splat(0.f);
    ierr[k] = splat(0.f);
  }
  float dbg_p = 0.f, dbg_i = 0.f, dbg_d = 0.f;
  bool dbg_wrote = false;
  if (run_pid) {
    // the DMA has landed once vmcnt reaches 0 (its LDS writes are counted there).  hipcc tracks an LDS-DMA against the
    // ds_reads of the same LDS object and places this wait by itself; it is spelled out anyway.  No "memory" clobber:
    // that would stop the derivative weights below from being scalar loads.  0x0F70 = vmcnt(0), expcnt / lgkmcnt untouched.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    CDPR_STAMP(4);
    if (kCmdLds) {
#pragma unroll
      for (int g = 0; g < kCmdRows; ++g) {
        const float4 v = stage[kCtrl + g][lane];
        desired[2 * g] = (v2f){v.x, v.y};
        desired[2 * g + 1] = (v2f){v.z, v.w};
      }
    }
    v2f win[NP][kWin];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const float4 w = stage[5 * k + m][lane];
        win[k][2 * m] = (v2f){w.x, w.y};
        win[k][2 * m + 1] = (v2f){w.z, w.w};
      }
    }
#pragma unroll
    for (int g = 0; g < NH; ++g) {
      const float4 h = stage[5 * NP + g][lane];
      ierr[2 * g] = (v2f){h.x, h.y};
      if (2 * g + 1 < NP) ierr[2 * g + 1] = (v2f){h.z, h.w};
    }
    const bool actual_is_vel = (a.flags & kFlagActualIsVelocity) != 0u;
    v2f actual[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) actual[k] = actual_is_vel ? qd[k] : q[k];
    const int ring_slot = a.ring_slot;
    pid_pairs<NP>(a, a.pid_calls, actual_is_vel, desired, actual, win, ierr, f, e_new, dbg_p, dbg_i, dbg_d);
    dbg_wrote = true;
    if (live) {  // one ring row per cable pair (the one that takes the new error) + the integral rows
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        if (m == (ring_slot >> 1)) {
#pragma unroll
          for (int k = 0; k < NP; ++k) CDPR_STORE_STATE(a.state, st, P + 5 * k + m, woff, ring_row(win[k], m, e_new[k], ring_slot));
        }
      }
#pragma unroll
      for (int g = 0; g < NH; ++g) {
        const int k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
        CDPR_STORE_STATE(a.state, st, P + 5 * NP + g, woff, make_float4(ierr[2 * g].x, ierr[2 * g].y, ierr[k1].x, ierr[k1].y));
      }
    }
  }

  if (force_mode && !first_world) {
#pragma unroll
    for (int k = 0; k < NP; ++k) f[k] = desired[k];
  }

  // ---- PERSIST: the staged rows have been read: request the next block's (controller rows and Joy by LDS-DMA into the
  //      same staging buffer, platform rows into registers); they arrive under this block's remaining stages
  if (PERSIST && more) {
    const uint32_t noff = nrr * 16u;
    if (run_pid) {
#pragma unroll
      for (int j = 0; j < kCtrl; ++j)
        row_to_lds(reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.state + (size_t)(P + j) * st) + noff), &stage[j][0]);
      if (kCmdLds) {
        const float* ncp = a.cmd + (size_t)nrr * N;
#pragma unroll
        for (int g = 0; g < kCmdRows; ++g) row_to_lds(reinterpret_cast<const float4*>(ncp) + g, &stage[kCtrl + g][0]);
      }
    }
  }

  CDPR_STAMP(5);
  // ---- tension distribution ([NEW] SURVEY 8(a) row 15), SetForce limits
  v2f applied[NP];
  int td_flag = 0;
  if (TD) {
    v2f df[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) df[k] = f[k] - splat(a.td_mid);
    float g[6];
    if (FK) {
      jt_times<NP>(jest, df, g);
      normal_solve<NP, false>(jest, 0.f, g);
    } else {
      jt_times<NP>(jac, df, g);
      normal_solve<NP, false>(jac, 0.f, g);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      v2f t = splat(a.td_mid);
#pragma unroll
      for (int c = 0; c < 6; ++c) t = fma2(g[c], FK ? jest[k][c] : jac[k][c], t);
      const v2f tc = max2(min2(t, splat(a.td_max)), splat(a.td_min));
      td_flag |= (tc.x != t.x) ? 1 : 0;
      if (2 * k + 1 < N) td_flag |= (tc.y != t.y) ? 1 : 0;
      applied[k] = tc;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NP; ++k) applied[k] = f[k];
  }
  setforce_limits<NP>(a, qd, applied);

  if (a.dbg && live) write_pid_topic(a.dbg + (size_t)r * 9, dbg_wrote, dbg_wrote, dbg_p, dbg_i, dbg_d, desired[0].x, applied[0].x);
  if (publish && live) {  // the rest of the observables
    store_slot(a.obs, st, 3, woff, make_float4(s.wz, fk_res, (float)fk_it, pack_flags(td_flag, travel_mask<N>(a, q))));
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k0 = 2 * g, k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
      const bool has = (2 * g + 1 < NP);
      store_slot(a.obs, st, 4 + 2 * G + g, woff,
                make_float4(applied[k0].x, applied[k0].y, has ? applied[k1].x : 0.f, has ? applied[k1].y : 0.f));
    }
  }

  CDPR_STAMP(6);
  // ---- world step to t_{k+1}: wrench = -J^T (applied - d qdot) + m g
  {
    v2f tens[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      tens[k] = fma2(-a.damping, qd[k], applied[k]);
      if (a.unilateral) tens[k] = max2(tens[k], splat(0.f));
    }
    if (FK) {
      // the true structure matrix did not live through the Newton stage: rebuild it (same inputs, same instructions,
      // same bits).  The geometry pointer is made opaque so the compiler cannot keep the first evaluation alive instead.
      uint32_t again = 0;  // an opaque zero OFFSET (an opaque pointer would lose the LDS address space: flat loads)
      asm volatile("" : "+v"(again));
      v2f len2[NP], l02[NP];
      ik_pairs<N, false>(lds + again, s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, len2, jac, l02);
    }
    float w[6];
    jt_times<NP>(jac, tens, w);
    w[0] = a.fgx - w[0];
    w[1] = a.fgy - w[1];
    w[2] = a.fgz - w[2];
    w[3] = -w[3];
    w[4] = -w[4];
    w[5] = -w[5];
    integrate(a, s, w);
  }
  if (PERSIST && more) {
    // the next block's rows are waited for HERE, before this block's last stores are issued: the compiler drains every
    // outstanding memory operation at the first use of a load's result while an LDS-DMA is pending, and at the top of
    // the next block that would include these stores
    // (everything issued before the last kDmaOps operations is complete: the platform rows went out before the DMA)
    constexpr int kDmaOps = kCtrl + kCmdRows;
    static_assert(kDmaOps < 64, "vmcnt is a 6-bit counter");
    if (run_pid)
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(kDmaOps));
    else
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    asm volatile("" : "+a"(n0), "+a"(n1), "+a"(n2), "+a"(n3), "+a"(n4));
  }
  if (live) {
    CDPR_STORE_STATE(a.state, st, 0, woff, make_float4(s.px, s.py, s.pz, s.qx));
    CDPR_STORE_STATE(a.state, st, 1, woff, make_float4(s.qy, s.qz, s.qw, s.vx));
    CDPR_STORE_STATE(a.state, st, 2, woff, make_float4(s.vy, s.vz, s.wx, s.wy));
    CDPR_STORE_STATE(a.state, st, 3, woff, make_float4(s.wz, fkx, fky, fkz));
    if (FK) CDPR_STORE_STATE(a.state, st, 4, woff, make_float4(fkqx, fkqy, fkqz, fkqw));
  }
  CDPR_STAMP(7);
  if (!(PERSIST && more)) break;
  blk = nblk;
  r = nr;
  rr = nrr;
  live = r < a.batch;
  off = rr * 16u, woff = r * 16u;
  p0 = make_float4(n0.x, n0.y, n0.z, n0.w), p1 = make_float4(n1.x, n1.y, n1.z, n1.w), p2 = make_float4(n2.x, n2.y, n2.z, n2.w);
  p3 = make_float4(n3.x, n3.y, n3.z, n3.w), p4 = make_float4(n4.x, n4.y, n4.z, n4.w);
  staged = run_pid;
  }  // blocks
}

// =====================================================================================================================
// cdpr_split_kernel — the one-step launch for FK + TD handles with TWO waves per 64 robots (a 128-thread workgroup), each
// with its own role, so that every SIMD hosts two waves although 65 536 robots are only 1 024 wavefronts of lanes:
//
//   estimator wave (wave 0)   platform rows -> measured lengths -> Newton-Raphson FK (4 iterations + closing evaluation)
//                             -> [forces from the controller wave] tension distribution -> tensions back
//   controller wave (wave 1)  platform + controller rows -> IK (structure matrix, joint positions / rates) -> early
//                             observables -> per-cable PID -> forces out -> [tensions from the estimator wave] SetForce
//                             limits -> remaining observables -> world step -> state
//
// Why: one wave issues a vector instruction every 5 cycles at best (8.3 when it needs its predecessor's result), while
// the SIMD takes a plain instruction every 2.5 cycles and a packed one every 4.2 (scripts/micro/valu_issue.hip): the
// scarce thing is the issue rate of the wave that carries a robot's serial chain, so everything that is not on that
// chain belongs on another (younger, lower-priority) wave that uses the slots the first leaves.  The lane-pair mapping gets its second wave by giving every robot two lanes, which
// duplicates the serial 6x6 solves (+46 % instructions: measured slower from 65 536 robots on).  Splitting by ROLE
// duplicates only the platform-row loads and one length evaluation (~3 %), and it takes the PID, the observable stores
// and all controller-row traffic off the Newton stage's critical path.  The hand-offs are 8 forces one way and 8
// tensions + 6 estimator scalars the other way, through LDS, with two workgroup barriers.  Same arithmetic as the
// one-wave kernels (shared device functions, -ffp-contract=off): bit-identical, tested.
// Registers: __launch_bounds__(128, 2) = at most 256 per wave, VGPR + AGPR together.
#ifndef CDPR_CTL_LOAD_DELAY
#define CDPR_CTL_LOAD_DELAY 8  // s_sleep units (64 cycles) the controller wave waits before it issues its 22 controller-row loads: the
#endif                         // estimator waves' two rows (the start of the serial chain) then meet a memory system that is not yet
                               // flooded by 2 048 x 27 row requests.  Interleaved A/Bs on three leases, us/step against 0: 4: 9.90-10.07
                               // vs 10.20-10.38; 6 / 8: 10.20-10.34 / 10.12-10.36 vs 10.50-10.72; 6 / 8 / 12: 10.27 / 10.26 / 10.20 vs
                               // 10.38 (medians); 16: no gain
#ifndef CDPR_SPLIT_PRIO
#define CDPR_SPLIT_PRIO 1  // 1 = estimator wave at s_setprio 3 (measured 10.89 vs 11.05 us/step), 2 = controller wave at 3 (11.7), 0 = none
#endif
#ifndef CDPR_STEADY_SHARED_IK
#define CDPR_STEADY_SHARED_IK 1  // 1 = the steady kernel evaluates the true-state IK once per robot (estimator wave, rows through LDS); 0 = both waves do
#endif
#ifndef CDPR_STEADY_NEWTON_WRITTEN_OUT
#define CDPR_STEADY_NEWTON_WRITTEN_OUT 1  // 1 = the steady kernel's Newton stage is four iterations written out; 0 = the generic loop (A/B of the two items)
#endif
#ifndef CDPR_EST_PIN_FACTOR
#define CDPR_EST_PIN_FACTOR 1  // 1 = the estimator wave (every instantiation) holds the tension distribution's factor in front of barrier #1 by an empty asm;
#endif                         //     0 = the compiler places it (A/B: scripts/build_variants.sh pin0)
#ifndef CDPR_STEADY_SHARED_ROT
#define CDPR_STEADY_SHARED_ROT 1  // 1 = with the shared IK the estimator wave hands the true state's rotation matrix over as well (nine rows through LDS)
#endif                            //     and the controller wave's world step takes it; 0 = the controller wave evaluates it behind barrier #2
constexpr int kIkRows = 7;  // v2f rows per cable pair of that hand-over: L, u (3), (R b) x u (3)
constexpr bool kSteadySharedRot = CDPR_STEADY_SHARED_IK && CDPR_STEADY_SHARED_ROT;

// The orientation of the estimator wave's pose estimate through the Newton stage, held as the pairs (x, y), (z, w) that quat_to_rot_pk and
// quat_apply_rotvec_pk work on (CDPR_QUAT_PK = 0: the scalar stages on the halves).  Row 4 of the state keeps its layout.
struct EstQuat {
  v2f a, b;
};
CDPR_DEV EstQuat est_quat(const float4& v) { return EstQuat{(v2f){v.x, v.y}, (v2f){v.z, v.w}}; }
CDPR_DEV float4 est_quat_row(const EstQuat& q) { return make_float4(q.a.x, q.a.y, q.b.x, q.b.y); }
template <int N>
CDPR_DEV void est_ik(const float* geo, float x, float y, float z, const EstQuat& q, v2f (&len)[cable_pairs(N)], v2f (&jac)[cable_pairs(N)][6],
                     v2f (&l0)[cable_pairs(N)]) {
#if CDPR_QUAT_PK
  ik_pairs_pk<N, false>(geo, x, y, z, quat_to_rot_pk(q.a, q.b), len, jac, l0);
#else
  ik_pairs<N, false>(geo, x, y, z, q.a.x, q.a.y, q.b.x, q.b.y, len, jac, l0);
#endif
}
CDPR_DEV void est_rotate(EstQuat& q, float tx, float ty, float tz) {
#if CDPR_QUAT_PK
  quat_apply_rotvec_pk(q.a, q.b, tx, ty, tz);
#else
  float x = q.a.x, y = q.a.y, z = q.b.x, w = q.b.y;
  quat_apply_rotvec(x, y, z, w, tx, ty, tz);
  q = EstQuat{(v2f){x, y}, (v2f){z, w}};
#endif
}
// The rotation matrix of the TRUE state's quaternion (rows 0 and 1 of the state) as the role-split waves form it, and the IK rows at the
// true state with it: the world step (integrate_velocity) takes the same matrix.
CDPR_DEV Rot true_state_rot(float qx, float qy, float qz, float qw) {
#if CDPR_QUAT_PK
  return unpack_rot(quat_to_rot_pk((v2f){qx, qy}, (v2f){qz, qw}));
#else
  return quat_to_rot(qx, qy, qz, qw);
#endif
}
template <int N, bool WANT_L0>
CDPR_DEV Rot true_state_ik(const float* geo, float px, float py, float pz, float qx, float qy, float qz, float qw, v2f (&len)[cable_pairs(N)],
                           v2f (&jac)[cable_pairs(N)][6], v2f (&l0)[cable_pairs(N)]) {
#if CDPR_QUAT_PK
  const RotPk r = quat_to_rot_pk((v2f){qx, qy}, (v2f){qz, qw});
  ik_pairs_pk<N, WANT_L0>(geo, px, py, pz, r, len, jac, l0);
  return unpack_rot(r);
#else
  ik_pairs<N, WANT_L0>(geo, px, py, pz, qx, qy, qz, qw, len, jac, l0);
  return quat_to_rot(qx, qy, qz, qw);  // (ik_pairs' own evaluation: the compiler keeps one)
#endif
}
#ifdef CDPR_STAMPS
#define CDPR_SPLIT_STAMP(i)                                                                                          \
  do {                                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    if (a.stamps && lane == 0) a.stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime();           \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
  } while (0)
#else
#define CDPR_SPLIT_STAMP(i) do { } while (0)
#endif
#if defined(CDPR_STAMPS) && defined(CDPR_STAMPS_ITER)  // stamps 4..6 = end of Newton iterations 1..3 instead of the controller's
#define CDPR_CTL_STAMP(i) do { } while (0)
#else
#define CDPR_CTL_STAMP(i) CDPR_SPLIT_STAMP(i)
#endif

// The estimator wave of a role-split workgroup (cdpr_split_kernel): platform rows -> measured lengths -> Newton-Raphson FK -> [forces from the controller wave] tension distribution
// -> tensions and estimator results back.  x_force / x_tension: v2f rows XS elements apart, x_est: float rows ES apart.
// RAISED: this wave at raised issue priority (the fast path's kernel: its chain is the launch's; the general kernels, whose controller
// wave is the longer one, pass their own choice)
//
// STEADY: the estimator half of cdpr_split_steady_kernel, for launches of which the host knows (split_steady_launch, cdpr_engine_launch.hip)
// besides the controller wave's facts that fk_tol == 0 and fk_iters == 4.  Every floating-point operation is the generic instantiation's, in
// its order and on its operands (same device functions, same bits: tested); two things differ.
//  1. The Newton stage is four iterations written out.  With a tolerance of 0 the generic loop's `active && !(rm < fk_tol)` is true for every
//     residual, NaN included: every lane moves and counts in every iteration, so the residual maximum inside the iterations, the mask
//     around the pose update and the counter (4) are gone.  The closing evaluation and fk_res stay.
//  2. (CDPR_STEADY_SHARED_IK) The IK rows at the true state are evaluated ONCE per robot, here: lengths, unit vectors and (R b) x u of
//     every pair go to x_ik (kIkRows v2f rows per pair, 64 lanes each) and this wave passes workgroup barrier #0.  The controller wave
//     issues its row loads, goes to #0 (it is there first: this wave does not wait) and reads the rows instead of calling ik_pairs; L0
//     comes from its geometry table.  The generic kernel evaluates them in both waves (the estimator needs the lengths only, so the
//     compiler drops its unit vectors and cross products there).
//  3. (CDPR_STEADY_SHARED_ROT, with 2) The rotation matrix of the true state's quaternion, which that IK evaluation forms, goes the same way: nine
//     float rows of 64 lanes (x_rot: r00 r01 r02 r10 .. r22, 2.25 KiB) written next to the IK rows in front of barrier #0.  The controller wave
//     reads them behind barrier #2 and gives them to integrate_velocity's overload instead of evaluating quat_to_rot in its tail.
//  4. The iteration count is not handed over: steady launches run four iterations, every one counts, so the controller wave publishes the
//     literal 4 and x_est row 4 is not written.
// In EVERY instantiation (CDPR_QUAT_PK) the orientation estimate is held through the Newton stage as the pairs (x, y), (z, w) (EstQuat) and the
// stages on it are the pair forms of cdpr_step_kernel.hpp - quat_to_rot_pk, ik_rows_pk, quat_apply_rotvec_pk: the scalar stages' operations on
// the same operands, bit for bit (tests/test_gpu_quat_stages.py holds them against the one-wave kernel, which keeps the scalar stages) - and the
// tension distribution's factor is pinned in front of barrier #1 (CDPR_EST_PIN_FACTOR, see there).
// Static counts of both waves, before and after: scripts/split_ctl_counts.py, profiles/r11_split_est_instruction_counts.txt (items 1, 2),
// profiles/r22_split_quat_instruction_counts.txt (item 3 and the pair forms).
// Measured per item (profiles/r11_headline_steady_estimator_ab.txt): 2 is the gain; 1 ALONE is no faster than the generic loop (the compiler then
// moves the tension distribution's factor behind barrier #1) and worth 0.1 us per step on top of 2.
template <int N, int XS, int ES, bool RAISED = true, bool STEADY = false>
CDPR_DEV void split_estimator_wave(const StepArgs& a, float* geo, float gval, uint32_t lane, bool live, size_t st, uint32_t off, uint32_t woff,
                                   const float4& p0, const float4& p1, const float4& p3, const v2f* x_force, v2f* x_tension, float* x_est,
                                   v2f* x_ik = nullptr, float* x_rot = nullptr) {
  constexpr int NP = cable_pairs(N);
#if defined(CDPR_STAMPS) && defined(CDPR_STAMPS_CLOCK)  // the shader clock over this wave: s_memtime ticks between entry and stamp 3, into slot 7
  const unsigned long long clk0 = __builtin_amdgcn_s_memtime();
#endif
#if CDPR_SPLIT_PRIO == 1 || CDPR_SPLIT_PRIO == 4
  if (RAISED) __builtin_amdgcn_s_setprio(3);  // the estimator is the critical path: it wins the SIMD's issue arbitration
#elif CDPR_SPLIT_PRIO == 3 || CDPR_SPLIT_PRIO == 5
  if (RAISED) __builtin_amdgcn_s_setprio(2);
#endif
  const float4 p4 = load_slot(a.state, st, 4, off);
  if (lane < NP * kGeomFloatsPerPair) geo[lane] = gval;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float fkx = p3.y, fky = p3.z, fkz = p3.w;
  EstQuat fkq = est_quat(p4);
  v2f len[NP];
  {
    v2f jac[NP][6], l0[NP];  // only the measured lengths L* are kept of the true-state evaluation
    float tqx = p0.w, tqy = p1.x, tqz = p1.y, tqw = p1.z;
#if CDPR_QUAT_PK
    // (the rows arrive in the kernel's prologue, which both waves run: left free, the compiler lines these four up as pairs THERE, and the
    //  controller wave carries two registers more through its PID stage, its register peak)
    asm volatile("" : "+v"(tqx), "+v"(tqy), "+v"(tqz), "+v"(tqw));
#endif
    const Rot r = true_state_ik<N, false>(geo, p0.x, p0.y, p0.z, tqx, tqy, tqz, tqw, len, jac, l0);
    if (STEADY && CDPR_STEADY_SHARED_IK) {  // ... and the whole of it goes to the controller wave, which evaluates none itself
      if (kSteadySharedRot) {  // ... with the matrix itself, which its world step needs (integrate_velocity)
        x_rot[0 * 64 + lane] = r.r00, x_rot[1 * 64 + lane] = r.r01, x_rot[2 * 64 + lane] = r.r02;
        x_rot[3 * 64 + lane] = r.r10, x_rot[4 * 64 + lane] = r.r11, x_rot[5 * 64 + lane] = r.r12;
        x_rot[6 * 64 + lane] = r.r20, x_rot[7 * 64 + lane] = r.r21, x_rot[8 * 64 + lane] = r.r22;
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        x_ik[(kIkRows * k) * 64 + lane] = len[k];
#pragma unroll
        for (int c = 0; c < 6; ++c) x_ik[(kIkRows * k + 1 + c) * 64 + lane] = jac[k][c];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the rows are in LDS
      __builtin_amdgcn_s_barrier();        // #0: the controller wave is here already (it has only issued its row loads)
    }
  }
  float fk_res = 0.f;
  int fk_it = 0;
  v2f jest[NP][6];
  {
    v2f elen[NP], unused[NP];
    if (STEADY && CDPR_STEADY_NEWTON_WRITTEN_OUT) {
      // fk_tol == 0 and fk_iters == 4 (split_steady_launch): `!(rm < 0)` holds for every residual, NaN included, so every lane moves
      // and counts in every iteration - the four iterations written out, without the test, the mask and the counter
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        est_ik<N>(geo, fkx, fky, fkz, fkq, elen, jest, unused);
        v2f res[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) res[k] = len[k] - elen[k];
        float g[6];
        jt_times<NP>(jest, res, g);
        normal_solve<NP>(jest, a.fk_lambda, g);
        fkx += g[0];
        fky += g[1];
        fkz += g[2];
        est_rotate(fkq, g[3], g[4], g[5]);
#ifdef CDPR_STAMPS_ITER
        if (it < 3) {
          asm volatile("" ::"v"(est_quat_row(fkq).w));
          __builtin_amdgcn_sched_barrier(0);
          if (a.stamps && lane == 0) a.stamps[(size_t)blockIdx.x * 8 + 4 + it] = __builtin_amdgcn_s_memrealtime();
          __builtin_amdgcn_sched_barrier(0);
        }
#endif
      }
      fk_it = 4;
    } else {
      bool active = true;
      for (int it = 0; it < a.fk_iters; ++it) {
        est_ik<N>(geo, fkx, fky, fkz, fkq, elen, jest, unused);
        v2f res[NP];
        v2f rm = splat(0.f);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          res[k] = len[k] - elen[k];
          rm = max2(rm, abs2(res[k]));
        }
        active = active && !(fmaxf(rm.x, rm.y) < a.fk_tol);
        float g[6];
        jt_times<NP>(jest, res, g);
        normal_solve<NP>(jest, a.fk_lambda, g);
        if (active) {
          fkx += g[0];
          fky += g[1];
          fkz += g[2];
          est_rotate(fkq, g[3], g[4], g[5]);
          ++fk_it;
        }
#ifdef CDPR_STAMPS_ITER
        if (it < 3) {
          asm volatile("" ::"v"(est_quat_row(fkq).w));
          __builtin_amdgcn_sched_barrier(0);
          if (a.stamps && lane == 0) a.stamps[(size_t)blockIdx.x * 8 + 4 + it] = __builtin_amdgcn_s_memrealtime();
          __builtin_amdgcn_sched_barrier(0);
        }
#endif
      }
    }
    est_ik<N>(geo, fkx, fky, fkz, fkq, elen, jest, unused);
    v2f rm = splat(0.f);
#pragma unroll
    for (int k = 0; k < NP; ++k) rm = max2(rm, abs2(len[k] - elen[k]));
    fk_res = fmaxf(rm.x, rm.y);
  }
  if (live) store_slot_aux<CDPR_SPLIT_PLAT_AUX>(a.state, st, 4, woff, est_quat_row(fkq));
  CDPR_SPLIT_STAMP(1);
  // the tension distribution's matrix and its factor need no forces: done while the controller wave may still be busy
  v2f td_l[6][3];
  float td_invd[6];
  normal_matrix_pk<NP, false>(jest, 0.f, td_l);
  chol_factor_pk(td_l, td_invd);
#if CDPR_EST_PIN_FACTOR
  // (pinned in front of the barrier: the last pivot has the whole factor and the closing evaluation's structure matrix upstream, the
  //  residual its lengths.  Left free, the compiler is at liberty to sink both behind barrier #1, onto the path after the force hand-off;
  //  with the pair forms in it does, in every instantiation: 131 -> 391 vector instructions between #1 and #2 at n = 8.)
  asm volatile("" ::"v"(td_invd[5]), "v"(fk_res));
#endif
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): nothing of this wave's LDS traffic is pending
  __builtin_amdgcn_s_barrier();        // #1: the controller wave's forces are in x_force
  CDPR_SPLIT_STAMP(2);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  v2f f[NP], df[NP], t_out[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    f[k] = x_force[k * XS + lane];
    df[k] = f[k] - splat(a.td_mid);
  }
  int td_flag = 0;
  {
    float g[6];
    jt_times<NP>(jest, df, g);
    chol_apply_pk(td_l, td_invd, g);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      v2f t = splat(a.td_mid);
#pragma unroll
      for (int c = 0; c < 6; ++c) t = fma2(g[c], jest[k][c], t);
      const v2f tc = max2(min2(t, splat(a.td_max)), splat(a.td_min));
      td_flag |= (tc.x != t.x) ? 1 : 0;
      if (2 * k + 1 < N) td_flag |= (tc.y != t.y) ? 1 : 0;
      t_out[k] = tc;
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) x_tension[k * XS + lane] = t_out[k];
  x_est[0 * ES + lane] = fkx;
  x_est[1 * ES + lane] = fky;
  x_est[2 * ES + lane] = fkz;
  x_est[3 * ES + lane] = fk_res;
  if (!STEADY) x_est[4 * ES + lane] = (float)fk_it;  // (steady launches run four iterations: the controller wave knows)
  x_est[5 * ES + lane] = (float)td_flag;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0xC07F);
  CDPR_SPLIT_STAMP(3);
#if defined(CDPR_STAMPS) && defined(CDPR_STAMPS_CLOCK)
  if (a.stamps && lane == 0) a.stamps[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memtime() - clk0;
#endif
  __builtin_amdgcn_s_barrier();  // #2: tensions and estimator results are out
}

// The controller wave of a role-split workgroup (cdpr_split_kernel): platform + controller rows -> IK (structure matrix, joint positions /
// rates) -> early observables -> per-cable PID -> forces out -> [tensions from the estimator wave] SetForce limits -> remaining
// observables -> world step -> state.  x_force / x_tension: v2f rows of 64, x_est: float rows of 64 (split_estimator_wave's XS = ES = 64).
//
// STEADY: the instantiation for launches of which the host knows (split_steady_launch, cdpr_engine.hip) that the handle is uniform and in
// Velocity (VEL) or Position mode, that this is not world step 0, that the derivative window is full (calls >= nbuf), that the step is
// published and that neither the `pid` topic nor the travel flags are on.  Every floating-point operation is the generic instantiation's,
// in its order and on its operands (same device functions, same bits: tested); what goes is what those facts make dead or wave-uniform:
// the selects on `full`, on the mode and on the first step with the zero defaults they choose from, the debug and travel-flag code, and
// with them the 14 spilled scalar registers (0 here, 234 VGPRs against 247).  The ring row's layout is a scalar branch on the launch's
// ring position (the compiler turns the half-row choice back into selects where that is shorter).  Measured and not in the tree: the
// rows through a buffer descriptor instead of a 64-bit address each, 0.2 us per step slower.  The clamps stay
// max(min()) pairs: v_med3_f32 returns the LOWER bound for a NaN operand where the pair returns the upper one, so it is not bit-equal
// for any of the bounds in use.
// The world step takes the rotation matrix of the true quaternion from where it was formed (integrate_velocity's overload): the generic
// instantiation from its own IK (true_state_ik: the pair form under CDPR_QUAT_PK; nine registers live across the PID stage, 247 -> 244 VGPRs
// at n = 8), the steady one from the estimator wave's nine x_rot rows behind barrier #2 (CDPR_STEADY_SHARED_ROT; = 0: it forms the matrix in its
// tail, as before).  STEADY: the iteration count it publishes is the literal 4 (the estimator wave hands none over).
template <int N, bool PR, bool STEADY, bool VEL>
CDPR_DEV void split_controller_wave(const StepArgs& a, float* geo, float gval, uint32_t lane, uint32_t r, uint32_t rr, bool live, size_t st, uint32_t off,
                                    uint32_t woff, const float4& p0, const float4& p1, const float4& p2, const float4& p3, v2f* x_force, const v2f* x_tension,
                                    const float* x_est, const v2f* x_ik = nullptr, const float* x_rot = nullptr) {
  static_assert(!(STEADY && PR), "the steady instantiation serves uniform handles");
  constexpr int NP = cable_pairs(N);
  constexpr int P = plat_slots(true);
  constexpr int G = joint_groups(N);
  constexpr int NH = (NP + 1) / 2;
#if CDPR_SPLIT_PRIO == 2 || CDPR_SPLIT_PRIO == 5
  __builtin_amdgcn_s_setprio(3);  // (5: from its first instruction to the force hand-off)
#endif
#if CDPR_CTL_LOAD_DELAY > 0
  __builtin_amdgcn_s_sleep(CDPR_CTL_LOAD_DELAY);  // the estimator waves' two rows go first through the memory system
#endif
  float4 wraw[NP][5], hraw[NH];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int m = 0; m < 5; ++m) wraw[k][m] = load_slot(a.state, st, P + 5 * k + m, off);
  }
#pragma unroll
  for (int g = 0; g < NH; ++g) hraw[g] = load_slot(a.state, st, P + 5 * NP + g, off);
  v2f desired[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) desired[k] = splat(0.f);
  const float* cp = a.cmd + (size_t)rr * N;  // never null: before the first Joy the latched buffer holds zeros
  if (N % 4 == 0) {
#pragma unroll
    for (int g = 0; g < N / 4; ++g) {
      const float4 v = reinterpret_cast<const float4*>(cp)[g];
      desired[2 * g] = (v2f){v.x, v.y};
      desired[2 * g + 1] = (v2f){v.z, v.w};
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i & 1)
        desired[i / 2].y = cp[i];
      else
        desired[i / 2].x = cp[i];
    }
  }
  if (lane < NP * kGeomFloatsPerPair) geo[lane] = gval;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  Platform s;
  unpack_platform(p0, p1, p2, p3.x, s);

  // ---- IK on the state at t_k; the structure matrix stays alive for the world step (this wave runs no Newton stage)
  v2f len[NP], q[NP], qd[NP], jac[NP][6];
  constexpr bool kOwnIk = !(STEADY && CDPR_STEADY_SHARED_IK);
  Rot rot;  // of the true state's quaternion: the IK's, kept for the world step
  {
    v2f l0[NP];
    if (!kOwnIk) {  // the estimator wave's rows (same function, same operands: same bits), L0 from the geometry table
      __builtin_amdgcn_s_barrier();         // #0: reached with nothing but the row loads issued, so the estimator wave never waits here
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        len[k] = x_ik[(kIkRows * k) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 6; ++c) jac[k][c] = x_ik[(kIkRows * k + 1 + c) * 64 + lane];
        l0[k] = *reinterpret_cast<const v2f*>(geo + k * kGeomFloatsPerPair + 12);
      }
    } else {
      rot = true_state_ik<N, true>(geo, s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, len, jac, l0);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      q[k] = l0[k] - len[k];
      qd[k] = -fma2(s.wz, jac[k][5], fma2(s.wy, jac[k][4], fma2(s.wx, jac[k][3],
                    fma2(s.vz, jac[k][2], fma2(s.vy, jac[k][1], splat(s.vx) * jac[k][0])))));
    }
  }
  const bool publish = STEADY || (a.publish_mask & 1ull) != 0ull;
  if (publish && live) {
    store_slot(a.obs, st, 0, woff, make_float4(s.px, s.py, s.pz, s.qx));
    store_slot(a.obs, st, 1, woff, make_float4(s.qy, s.qz, s.qw, s.vx));
    store_slot(a.obs, st, 2, woff, make_float4(s.vy, s.vz, s.wx, s.wy));
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k0 = 2 * g, k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
      const bool has = (2 * g + 1 < NP);
      store_slot(a.obs, st, 4 + g, woff, make_float4(q[k0].x, q[k0].y, has ? q[k1].x : 0.f, has ? q[k1].y : 0.f));
      store_slot(a.obs, st, 4 + G + g, woff, make_float4(qd[k0].x, qd[k0].y, has ? qd[k1].x : 0.f, has ? qd[k1].y : 0.f));
    }
  }

  // ---- per-cable force (PLG.cpp:222-228 -> JFC.cpp:59-96 -> Pid.cpp:122-191)
  v2f f[NP], e_new[NP], ierr[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    f[k] = splat(0.f);
    e_new[k] = splat(0.f);
    ierr[k] = (k & 1) ? (v2f){hraw[k / 2].z, hraw[k / 2].w} : (v2f){hraw[k / 2].x, hraw[k / 2].y};
  }
  float dbg_p = 0.f, dbg_i = 0.f, dbg_d = 0.f;
  bool dbg_wrote = false;
  const bool first_world = !STEADY && (a.flags & kFlagFirstWorldStep) != 0u;
  uint32_t meta = 0u;
  if (PR) meta = a.meta[rr];
  const int calls = PR ? (int)(meta >> kMetaCallShift) : a.pid_calls;
  if (PR && live && !first_world) a.meta[r] = (uint8_t)((meta & kMetaModeMask) | ((uint32_t)min(calls + 1, (int)kMetaCallMax) << kMetaCallShift));
  const bool force_mode = !STEADY && !PR && (a.flags & kFlagForceMode) != 0u;  // UpdateMode::Force on a uniform handle (JFC.cpp:67-70)
  if (force_mode && !first_world) {
#pragma unroll
    for (int k = 0; k < NP; ++k) f[k] = desired[k];
  } else if (STEADY || (!first_world && (PR || calls != 0))) {
    v2f win[NP][kWin];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        win[k][2 * m] = (v2f){wraw[k][m].x, wraw[k][m].y};
        win[k][2 * m + 1] = (v2f){wraw[k][m].z, wraw[k][m].w};
      }
    }
    const bool actual_is_vel = STEADY ? VEL : PR ? ((meta & kMetaModeMask) == kMetaVelocity) : ((a.flags & kFlagActualIsVelocity) != 0u);
    v2f actual[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) actual[k] = actual_is_vel ? qd[k] : q[k];
    const int ring_slot = a.ring_slot;
    const bool is_force = PR && (meta & kMetaModeMask) == kMetaForce;
#if CDPR_SPLIT_PRIO == 3 || CDPR_SPLIT_PRIO == 4
    __builtin_amdgcn_s_setprio(3);  // (experiment) the forces are what the estimator wave will wait for
#endif
    pid_pairs<NP, PR, STEADY>(a, calls, actual_is_vel, desired, actual, win, ierr, f, e_new, dbg_p, dbg_i, dbg_d, is_force);
    dbg_wrote = (!PR || calls != 0) && !is_force;
    if (live) {
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        if (m == (ring_slot >> 1)) {
          if (!STEADY) {
#pragma unroll
            for (int k = 0; k < NP; ++k) CDPR_STORE_STATE(a.state, st, P + 5 * k + m, woff, ring_row(win[k], m, e_new[k], ring_slot));
          } else if (ring_slot & 1) {  // the row's layout by a scalar branch: the new error in the upper half ...
#pragma unroll
            for (int k = 0; k < NP; ++k) CDPR_STORE_STATE(a.state, st, P + 5 * k + m, woff, make_float4(win[k][2 * m].x, win[k][2 * m].y, e_new[k].x, e_new[k].y));
          } else {  // ... or in the lower one
#pragma unroll
            for (int k = 0; k < NP; ++k) CDPR_STORE_STATE(a.state, st, P + 5 * k + m, woff, make_float4(e_new[k].x, e_new[k].y, win[k][2 * m + 1].x, win[k][2 * m + 1].y));
          }
        }
      }
#pragma unroll
      for (int g = 0; g < NH; ++g) {
        const int k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
        CDPR_STORE_STATE(a.state, st, P + 5 * NP + g, woff, make_float4(ierr[2 * g].x, ierr[2 * g].y, ierr[k1].x, ierr[k1].y));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) x_force[k * 64 + lane] = f[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the forces are in LDS (vector memory operations stay in flight)
  CDPR_CTL_STAMP(4);
#if CDPR_SPLIT_PRIO >= 3
  __builtin_amdgcn_s_setprio(0);
#endif
  __builtin_amdgcn_s_barrier();        // #1
  __builtin_amdgcn_s_barrier();        // #2: the estimator wave has finished the tension distribution
  CDPR_CTL_STAMP(5);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  v2f applied[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) applied[k] = x_tension[k * 64 + lane];
  const float fkx = x_est[0 * 64 + lane], fky = x_est[1 * 64 + lane], fkz = x_est[2 * 64 + lane], fk_res = x_est[3 * 64 + lane],
              fk_it = STEADY ? 4.f : x_est[4 * 64 + lane], td_flag = x_est[5 * 64 + lane];  // (steady launches: fk_iters == 4, every one runs)
  if (!kOwnIk) {
    if (kSteadySharedRot) {  // the estimator wave's matrix (same function, same operands: same bits)
      rot = Rot{x_rot[0 * 64 + lane], x_rot[1 * 64 + lane], x_rot[2 * 64 + lane], x_rot[3 * 64 + lane], x_rot[4 * 64 + lane],
                x_rot[5 * 64 + lane], x_rot[6 * 64 + lane], x_rot[7 * 64 + lane], x_rot[8 * 64 + lane]};
    } else {
      rot = true_state_rot(s.qx, s.qy, s.qz, s.qw);
    }
  }
  setforce_limits<NP>(a, qd, applied);
  if (!STEADY && a.dbg && live) write_pid_topic(a.dbg + (size_t)r * 9, dbg_wrote, dbg_wrote, dbg_p, dbg_i, dbg_d, desired[0].x, applied[0].x);
  if (publish && live) {
    store_slot(a.obs, st, 3, woff, make_float4(s.wz, fk_res, fk_it, (!STEADY && a.travel_on) ? pack_flags((int)td_flag, travel_mask<N>(a, q)) : td_flag));
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k0 = 2 * g, k1 = (2 * g + 1 < NP) ? 2 * g + 1 : 2 * g;
      const bool has = (2 * g + 1 < NP);
      store_slot(a.obs, st, 4 + 2 * G + g, woff,
                 make_float4(applied[k0].x, applied[k0].y, has ? applied[k1].x : 0.f, has ? applied[k1].y : 0.f));
    }
  }
  // ---- world step to t_{k+1}: wrench = -J^T (applied - d qdot) + m g
  {
    v2f tens[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      tens[k] = fma2(-a.damping, qd[k], applied[k]);
      if (a.unilateral) tens[k] = max2(tens[k], splat(0.f));
    }
    float w[6];
    jt_times<NP>(jac, tens, w);
    w[0] = a.fgx - w[0];
    w[1] = a.fgy - w[1];
    w[2] = a.fgz - w[2];
    w[3] = -w[3];
    w[4] = -w[4];
    w[5] = -w[5];
    integrate(a, s, w, rot);
  }
  if (live) {
    store_slot_aux<CDPR_SPLIT_PLAT_AUX>(a.state, st, 0, woff, make_float4(s.px, s.py, s.pz, s.qx));
    store_slot_aux<CDPR_SPLIT_PLAT_AUX>(a.state, st, 1, woff, make_float4(s.qy, s.qz, s.qw, s.vx));
    store_slot_aux<CDPR_SPLIT_PLAT_AUX>(a.state, st, 2, woff, make_float4(s.vy, s.vz, s.wx, s.wy));
    store_slot_aux<CDPR_SPLIT_PLAT_AUX>(a.state, st, 3, woff, make_float4(s.wz, fkx, fky, fkz));
  }
  CDPR_CTL_STAMP(6);
}

// PR = true: per-robot handles (StepArgs::meta, see cdpr_step_kernel.hpp): the controller wave takes mode and Pid call
// count per lane; the estimator wave is the same.
// (the kernel's body: cdpr_split_kernel<N, PR> and cdpr_split_steady_kernel<N, VEL> below differ in the two waves' STEADY instantiations and
// in the LDS rows of the shared IK, which only the steady kernel has)
template <int N, bool PR, bool STEADY, bool VEL>
CDPR_DEV void split_kernel_body(const StepArgs& a) {
  constexpr int NP = cable_pairs(N);
  __shared__ __attribute__((aligned(16))) float lds[2][NP * kGeomFloatsPerPair];  // one geometry copy per wave: no barrier before first use
  __shared__ v2f x_force[NP][64];      // controller -> estimator: raw per-cable forces
  __shared__ v2f x_tension[NP][64];    // estimator -> controller: distributed tensions (before the SetForce limits)
  __shared__ float x_est[6][64];       // estimator -> controller: fk x y z, residual, iterations, infeasible flag
  v2f* x_ik = nullptr;                 // estimator -> controller, steady kernel only: the IK rows at the true state (14 KiB at n = 8)
  float* x_rot = nullptr;              // ... and its rotation matrix, nine rows (2.25 KiB)
  if constexpr (STEADY && CDPR_STEADY_SHARED_IK) {
    __shared__ v2f ik_rows_at_state[kIkRows * NP][64];
    x_ik = &ik_rows_at_state[0][0];
    if constexpr (kSteadySharedRot) {
      __shared__ float rot_at_state[9][64];
      x_rot = &rot_at_state[0][0];
    }
  }

  // which of the two waves estimates: swapped from workgroup to workgroup (bits of the workgroup index chosen by the
  // host, StepArgs::split_swap) so that the two waves a SIMD hosts tend to be one of each role
  const uint32_t swap = __builtin_popcount(blockIdx.x & a.split_swap) & 1u;
  const uint32_t wave = (threadIdx.x >> 6) ^ swap, lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * 64u + lane;
  const uint32_t rr = (r < a.batch) ? r : (a.batch - 1u);  // tail lanes shadow the last robot, stores are masked
  const bool live = r < a.batch;
  const size_t st = a.stride;
  const uint32_t off = rr * 16u, woff = r * 16u;
  float* const geo = lds[wave];

  if (wave == 0) CDPR_SPLIT_STAMP(0);
#ifdef CDPR_STAMPS
  if (a.stamps && lane == 0)  // where this wave runs: HW_ID (wave, SIMD, CU, SH, SE) | XCC_ID << 16, per PHYSICAL wave of the workgroup
    reinterpret_cast<uint32_t*>(&a.stamps[(size_t)blockIdx.x * 8 + 7])[threadIdx.x >> 6] =
        (__builtin_amdgcn_s_getreg((16 - 1) << 11 | 4) & 0xffffu) | ((__builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) & 0xfu) << 16);
#endif
  const float gval = (lane < NP * kGeomFloatsPerPair) ? a.geom[lane] : 0.f;
  const float4 p0 = load_slot(a.state, st, 0, off), p1 = load_slot(a.state, st, 1, off), p2 = load_slot(a.state, st, 2, off),
               p3 = load_slot(a.state, st, 3, off);
  if (wave == 0) {
    split_estimator_wave<N, 64, 64, true, STEADY>(a, geo, gval, lane, live, st, off, woff, p0, p1, p3, &x_force[0][0], &x_tension[0][0], &x_est[0][0], x_ik, x_rot);
    return;
  }
  split_controller_wave<N, PR, STEADY, VEL>(a, geo, gval, lane, r, rr, live, st, off, woff, p0, p1, p2, p3, &x_force[0][0], &x_tension[0][0], &x_est[0][0], x_ik, x_rot);
}
template <int N, bool PR = false>
__global__ __launch_bounds__(128, 2) void cdpr_split_kernel(const StepArgs a) { split_kernel_body<N, PR, false, false>(a); }
// The same kernel with both waves' steady-state instantiations (split_controller_wave<N, false, true, VEL>, split_estimator_wave<..., true>):
// the host's choice per launch (split_steady_launch, cdpr_engine_launch.hip), reported under cdpr_split_kernel<N, false>'s name by cdpr_kernel_name.
template <int N, bool VEL>
__global__ __launch_bounds__(128, 2) void cdpr_split_steady_kernel(const StepArgs a) { split_kernel_body<N, false, true, VEL>(a); }

}  // namespace cdpr
