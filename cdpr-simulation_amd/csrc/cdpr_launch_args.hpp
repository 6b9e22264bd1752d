// cdpr_launch_args.hpp - from a configuration to the bytes a kernel receives: pure functions of (cdpr_config_t, KernelPlan, mode), no HIP
// call, no handle (beside cdpr_select.hpp, which is the same for the routing).  cdpr_create calls launch_args() once, binds the handle's
// device pointers into the records (bind_args, cdpr_engine.hip) and uploads the tables; args_check.hip and cdpr_debug_launch_args run the
// same builders without a device.
//
// One Pid is one PidTerms, computed in double from cdpr_pid_params_t; every device-facing shape of it is written from that record by one
// function below (pid_set, write_pid, gen_pid, gen_tables, write_pid64, write_alt64, write_hold64, rotated_weights).  No other host
// code reads a gain, a limit or a filter out of cfg.velocity_pid / cfg.position_pid.
//
// A handle keeps one argument record per mode a uniform handle can be in, and one for a per-robot handle (args_index).  A launch site
// copies the record of the current mode and assigns ONLY what belongs to the call or the launch:
//   * the latched command pointer(s) of a uniform handle: StepArgs::cmd, F64Args::cmd, GenCtl::vel_cmd / pos_cmd / frc_cmd (they move
//     with every swap or bind);
//   * nsteps, kFlagFirstWorldStep (ORed onto the record's mode bits; rollouts: kFlagRolloutResetPid, schedules: kFlagPublishAll),
//     publish_mask, pid_calls, ring_slot, wrow;
//   * a trajectory record's obs and obs_step_stride, the sched_* fields with `fault`, the roll_* fields;
//   * GenCtl::now_step / F64Args::step0;
//   * rollouts and the warm launch of cdpr_create, which step scratch copies: the scratch's state (obs, cmd, meta, GenCtl::rec with
//     rstride / rec_bytes / src_rec / src_rstride; no `pid` topic: dbg = null), its stride and batch; launch_step: the chunk's rows.
// Everything else - travel_stop included - is complete in the record.
#pragma once
#include <cstring>
#include <vector>

#include "cdpr_kernels.hpp"

namespace cdpr_host {
using namespace cdpr;

// the argument structs are the kernels' ABI: a layout change is a change of every kernel, not of this header
static_assert(sizeof(PidSet) == 40 && sizeof(StepArgs) == 480 && sizeof(GenPid) == 92 && sizeof(GenCtl) == 136 && sizeof(F64Args) == 1320,
              "a kernel argument struct changed size");

enum Mode { kModeForce = 0, kModePosition = 1, kModeVelocity = 2 };  // JFC.h:35-37
enum { kPidPosition = 0, kPidVelocity = 1 };                           // as the kernels number the two Pids (GenCtl::ptab, F64Args::pcas ...)
constexpr int kArgsPerRobot = 3, kArgsRecords = 4;                     // records: one per Mode, then the per-robot handle's
inline int args_index(const KernelPlan& plan, int mode) { return plan.per_robot ? kArgsPerRobot : mode; }
// precision = 64: prior errors kept per cable (the ring of the handle's kernels), and the samples a HOLD record's window holds
inline int win64(const KernelPlan& plan) { return plan.long64 ? kWinLong : kWin; }
inline int hold_win(const KernelPlan& plan) { return plan.hold_long ? kHoldWinLong : kHoldWin; }

// Least-squares end-point derivative weights on a uniform grid, oldest sample first: the closed form of Pid::derive + fitPolynomial
// (Pid.cpp:193-247) when samples are one step apart.
inline int derivative_weights(uint32_t n, uint32_t degree, double* w) {
  if (n < 2 || n > CDPR_MAX_D_BUFFER || degree < 1 || degree > CDPR_MAX_D_DEGREE || degree >= n) return CDPR_ERR_INVALID;
  const int m = (int)degree + 1;
  long double a[5][10];  // [XtX | I], centred abscissae x_j = j - (n-1)/2
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < 2 * m; ++j) a[i][j] = 0.0L;
  std::vector<long double> x(n);
  for (uint32_t j = 0; j < n; ++j) x[j] = (long double)j - (long double)(n - 1) / 2.0L;
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k < m; ++k) {
      long double s = 0;
      for (uint32_t j = 0; j < n; ++j) s += powl(x[j], i + k);
      a[i][k] = s;
    }
    a[i][m + i] = 1.0L;
  }
  for (int col = 0; col < m; ++col) {  // Gauss-Jordan, partial pivoting
    int piv = col;
    for (int r = col + 1; r < m; ++r)
      if (fabsl(a[r][col]) > fabsl(a[piv][col])) piv = r;
    if (piv != col)
      for (int k = 0; k < 2 * m; ++k) std::swap(a[piv][k], a[col][k]);
    long double d = a[col][col];
    for (int k = 0; k < 2 * m; ++k) a[col][k] /= d;
    for (int r = 0; r < m; ++r) {
      if (r == col) continue;
      long double f = a[r][col];
      for (int k = 0; k < 2 * m; ++k) a[r][k] -= f * a[col][k];
    }
  }
  // derivative at the newest sample x_e: sum_k k x_e^(k-1) c_k, c = (XtX)^-1 Xt y
  const long double xe = x[n - 1];
  for (uint32_t j = 0; j < n; ++j) {
    long double wj = 0;
    for (int k = 1; k < m; ++k) {
      long double ck = 0;  // row k of (XtX)^-1 Xt, column j
      for (int i = 0; i < m; ++i) ck += a[k][m + i] * powl(x[j], i);
      wj += (long double)k * powl(xe, k - 1) * ck;
    }
    w[j] = (double)wj;
  }
  return CDPR_OK;
}

// BiQuad::SetFc(fc, fs = 1.0, q), Filter.h:130-140, in double: a0 a1 a2 b1 b2
inline void biquad_coefficients(const cdpr_filter_params_t& f, double co[5]) {
  const double k = std::tan(M_PI * f.rel_cutoff / 1.0);
  const double den = k * k + k / f.quality + 1.0;
  co[0] = k * k / den, co[1] = 2.0 * co[0], co[2] = co[0];
  co[3] = 2.0 * (k * k - 1.0) / den, co[4] = (k * k - k / f.quality + 1.0) / den;
}

// What one Pid contributes to any kernel, in double: the only place the rules of Pid.cpp:64-73 are stated on the host.
struct PidTerms {
  double kf, kp, ki, kd, inv_ki;   // inv_ki: 0 where ki == 0
  double imax, imin, cmax, cmin;   // +-|i_limit|, +-|cmd_limit| (Pid.cpp:70-73: abs -> fabs)
  int clamp, clamp32;              // cmax > cmin, as the fp64 and (limits rounded to float first) the fp32 kernels take it
  int nbuf, degree, pcas, dcas;
  double pco[5], dco[5];           // the P-input and D-input filters' a0 a1 a2 b1 b2, zeros where a filter has no stage
  double w[CDPR_MAX_D_BUFFER];     // uniform-grid derivative weights, oldest first
  int w_ok;                        // derivative_weights accepted (nbuf, degree)
};
inline PidTerms pid_terms(const cdpr_pid_params_t& p) {
  PidTerms t;
  memset(&t, 0, sizeof t);
  t.kf = p.forward_gain, t.kp = p.p_gain, t.ki = p.i_gain, t.kd = p.d_gain;
  t.inv_ki = (p.i_gain != 0.0) ? 1.0 / p.i_gain : 0.0;
  t.imax = std::fabs(p.i_limit), t.imin = -t.imax;
  t.cmax = std::fabs(p.cmd_limit), t.cmin = -t.cmax;
  t.clamp = t.cmax > t.cmin, t.clamp32 = (float)t.cmax > (float)t.cmin;
  t.nbuf = (int)p.d_buffer_length, t.degree = (int)p.d_degree;
  t.pcas = (int)p.p_filter.cascade, t.dcas = (int)p.d_filter.cascade;
  if (t.pcas) biquad_coefficients(p.p_filter, t.pco);
  if (t.dcas) biquad_coefficients(p.d_filter, t.dco);
  t.w_ok = derivative_weights(p.d_buffer_length, p.d_degree, t.w) == CDPR_OK;
  return t;
}

// ---- the fp32 shapes: PidSet (StepArgs::alt), the StepArgs primary fields, GenPid with its LDS table row
inline PidSet pid_set(const PidTerms& t) {
  return PidSet{(float)t.kf, (float)t.kp, (float)t.ki, (float)t.kd, (float)t.inv_ki, (float)t.imax, (float)t.imin, (float)t.cmax, (float)t.cmin, t.clamp32};
}
inline void write_pid(const PidTerms& t, StepArgs& a) {
  const PidSet s = pid_set(t);
  a.kf = s.kf, a.kp = s.kp, a.ki = s.ki, a.kd = s.kd, a.inv_ki = s.inv_ki;
  a.imax = s.imax, a.imin = s.imin, a.cmax = s.cmax, a.cmin = s.cmin;
  a.nbuf = t.nbuf, a.clamp_cmd = s.clamp_cmd;
}
inline GenPid gen_pid(const PidTerms& t) {
  const PidSet s = pid_set(t);
  return GenPid{s.kf, s.kp, s.ki, s.kd, s.imax, s.imin, s.cmax, s.cmin, t.nbuf, t.degree, t.pcas, t.dcas, s.clamp_cmd,
                (float)t.pco[0], (float)t.pco[1], (float)t.pco[2], (float)t.pco[3], (float)t.pco[4],
                (float)t.dco[0], (float)t.dco[1], (float)t.dco[2], (float)t.dco[3], (float)t.dco[4]};
}
// The general path's two uploaded tables.  ptab: both Pids as the kernel stages them in LDS (gen_pid_table), the last float of a row
// the FIR weight of the newest sample.  wtab: FIR weights by ring head, [pid][head][slot]: when the newest sample sits in slot `head`,
// slot j holds the sample of age (head - j) mod nbuf, whose end-point LS weight (oldest first) is w[nbuf - 1 - age]; slots >= nbuf weigh
// nothing, and neither does the head slot itself: the newest sample is still in a register when the FIR runs.
inline void gen_tables(const PidTerms pid[2], int nb, std::vector<float>& ptab, std::vector<float>& wtab) {
  const int nbmax = nb > 11 ? kGenMaxBuf : 11, nbp = gen_nbp(nbmax);
  ptab.assign((size_t)2 * kGenPidFloats, 0.f);
  wtab.assign((size_t)2 * nbmax * nbp, 0.f);
  for (int p = 0; p < 2; ++p) {
    gen_pid_table(gen_pid(pid[p]), &ptab[(size_t)p * kGenPidFloats]);
    const int n = pid[p].nbuf;
    if (!pid[p].w_ok) continue;
    for (int head = 0; head < n; ++head)
      for (int j = 0; j < n; ++j) wtab[((size_t)p * nbmax + head) * nbp + j] = (j == head) ? 0.f : (float)pid[p].w[n - 1 - (((head - j) % n + n) % n)];
    ptab[(size_t)(p + 1) * kGenPidFloats - 1] = (float)pid[p].w[n - 1];
  }
}

// A Pid's weights rotated per ring position, as T, for a ring of W errors: row ws (W + 2 entries) serves the launch whose new error goes
// to slot ws.  Slot (ws - j) mod W then holds the error of j steps ago (j = 1 .. W; j = W is slot ws itself, the sample about to be
// overwritten), whose weight is wpad[W - j]; entry W is the weight of the new error itself.
template <typename T>
void rotated_weights(const PidTerms& t, int W, T* tab) {
  std::vector<T> wpad((size_t)W + 1, (T)0);  // oldest..newest, zero padded at the old end to W + 1 entries
  if (t.w_ok && t.nbuf <= W + 1)
    for (int j = 0; j < t.nbuf; ++j) wpad[(size_t)(W + 1 - t.nbuf + j)] = (T)t.w[j];
  for (int ws = 0; ws < W; ++ws) {
    for (int s = 0; s < W; ++s) {
      int j = ((ws - s) % W + W) % W;
      if (j == 0) j = W;
      tab[ws * (W + 2) + s] = wpad[(size_t)W - j];
    }
    tab[ws * (W + 2) + W] = wpad[(size_t)W];
    tab[ws * (W + 2) + W + 1] = (T)0;
  }
}

template <typename T>
void rotated_tables(const PidTerms pid[2], int W, std::vector<T>& tab) {  // [velocity | position]
  tab.assign((size_t)2 * W * (W + 2), (T)0);
  rotated_weights(pid[kPidVelocity], W, &tab[0]);
  rotated_weights(pid[kPidPosition], W, &tab[(size_t)W * (W + 2)]);
}

// ---- the fp64 shapes: the F64Args primary fields, the alt_* fields (per-robot and HOLD handles: the position Pid), the hold fields
inline void write_pid64(const PidTerms& t, F64Args& a) {
  a.kf = t.kf, a.kp = t.kp, a.ki = t.ki, a.kd = t.kd, a.imax = t.imax, a.imin = t.imin, a.cmax = t.cmax, a.cmin = t.cmin;
  a.nbuf = t.nbuf, a.clamp_cmd = t.clamp;
}
inline void write_alt64(const PidTerms& t, F64Args& a) {
  a.alt_kf = t.kf, a.alt_kp = t.kp, a.alt_ki = t.ki, a.alt_kd = t.kd, a.alt_imax = t.imax, a.alt_imin = t.imin, a.alt_cmax = t.cmax, a.alt_cmin = t.cmin;
  a.alt_clamp_cmd = t.clamp;
}
// (pid[kPidVelocity] is in the primary fields, pid[kPidPosition] in alt_*; hold_win: the samples a HOLD record's window holds)
inline void write_hold64(const PidTerms pid[2], int hold_win, F64Args& a) {
  a.degree = pid[kPidVelocity].degree, a.alt_degree = pid[kPidPosition].degree, a.alt_nbuf = pid[kPidPosition].nbuf;
  a.any_noclamp = (!pid[0].clamp || !pid[1].clamp) ? 1 : 0;
  for (int t = 0; t < 2; ++t) {
    memcpy(a.pcoef[t], pid[t].pco, sizeof a.pcoef[t]);
    memcpy(a.dcoef[t], pid[t].dco, sizeof a.dcoef[t]);
    a.pcas[t] = std::min(pid[t].pcas, kHoldMaxCas), a.dcas[t] = std::min(pid[t].dcas, kHoldMaxCas);
    a.max_cas = std::max(a.max_cas, std::max(a.pcas[t], a.dcas[t]));
    for (int age = 0; pid[t].w_ok && age < pid[t].nbuf && age < hold_win; ++age) a.hold_w[t][age] = pid[t].w[pid[t].nbuf - 1 - age];  // by AGE of the sample
  }
  a.any_cas = a.max_cas > 0 ? 1 : 0;
}

// The world / body / FK / TD constants StepArgs (T = float) and F64Args (T = double) share: every value is computed in double
// and then cast.
template <typename T, typename Args>
void fill_physics(const cdpr_config_t& c, Args& k) {
  k.dt = (T)c.dt;
  k.half_dt = (T)(0.5 * c.dt);
  k.inv_dt = (T)(1.0 / c.dt);
  k.inv_mass = (T)(1.0 / c.mass);
  k.fgx = (T)(c.mass * c.gravity[0]);
  k.fgy = (T)(c.mass * c.gravity[1]);
  k.fgz = (T)(c.mass * c.gravity[2]);
  double inv[6];
  mat3_inverse_sym(c.inertia, inv);
  for (int i = 0; i < 6; ++i) {
    k.ib[i] = (T)c.inertia[i];
    k.ibinv[i] = (T)inv[i];
  }
  k.damping = (T)c.joint_damping;
  k.effort = (T)c.effort_limit;
  k.vel_limit = (T)c.velocity_limit;
  k.unilateral = c.unilateral_cables ? 1 : 0;
  k.travel_lo = (T)c.travel_lower;
  k.travel_hi = (T)c.travel_upper;
  k.travel_on = (c.travel_lower != 0.0 || c.travel_upper != 0.0) ? 1 : 0;
  k.ph_lumped = lumped_legs_on(c) ? 1 : 0;
  k.ph_c = (T)c.passive_damping;
  k.ph_jleg = (T)c.leg_inertia;
  k.ph_max = (T)c.cable_axial_mass;
  k.ph_mpt = (T)c.anchor_point_mass;
  k.ph_iadd_total = (T)(c.anchor_inertia * (double)c.n_cables);
  k.ph_mass = (T)c.mass;
  k.gx = (T)c.gravity[0];
  k.gy = (T)c.gravity[1];
  k.gz = (T)c.gravity[2];
  k.fk_lambda = (T)c.fk_lambda;
  k.fk_tol = (T)c.fk_tolerance;
  k.fk_iters = (int)c.fk_max_iterations;
  k.td_min = (T)c.td_f_min;
  k.td_max = (T)c.td_f_max;
  k.td_mid = (T)(0.5 * (c.td_f_min + c.td_f_max));
}

// Everything cdpr_create derives from the configuration for the handle's launches.
struct LaunchArgs {
  PidTerms pid[2];              // [kPidPosition], [kPidVelocity]
  StepArgs step[kArgsRecords];  // every handle: the constants (the solvers read step[0]); register-resident path: the launch's arguments
  GenCtl gen[kArgsRecords];     // general path: the controller half of a launch
  F64Args f64[kArgsRecords];    // precision = 64
  GenLayout glay;               // general path: rows of a Pid block, sized by the configured window length and cascade count
  std::vector<float> wtab;      // register-resident path: [velocity | position] rotated weight tables, kWin * (kWin + 2) floats each
                                // (uploaded; one-step launches take their row from here by value)
  std::vector<float> ptab, gwtab;  // general path: gen_tables
  std::vector<double> wtab64;      // precision = 64: [velocity | position] x [W][W + 2]
};

// The register-resident path's arguments in the record `rec`; general-path and precision = 64 handles: the constants alone.
inline StepArgs step_record(const cdpr_config_t& c, const KernelPlan& plan, const PidTerms pid[2], int rec, EnvFn env) {
  StepArgs a;
  memset(&a, 0, sizeof a);
  fill_physics<float>(c, a);
  a.dt_inv_mass = (float)(c.dt / c.mass);
  a.travel_stop = a.travel_on ? (int)c.travel_stop : 0;
  a.split_swap = 0x9;  // measured on MI355X (65 536 x 8): masks 0 .. 0xf8 give 10.8-11.3 us/step, 0x9 the best; bits 8-9 (the
                       // workgroups that share a CU) make it 12.8: the dispatcher already alternates the SIMD pairs there
  if (const char* sw = env("CDPR_SPLIT_SWAP")) a.split_swap = (uint32_t)strtoul(sw, nullptr, 0);
  if (plan.general || plan.fp64) return a;
  // per-robot kernels: the velocity Pid in the primary fields, the position Pid rides along as `alt`, the mode per lane (meta); a
  // uniform handle: the mode's Pid (Force: no Pid runs) and flag bits
  write_pid(pid[rec == kArgsPerRobot || rec == kModeVelocity], a);
  if (rec == kArgsPerRobot) a.alt = pid_set(pid[kPidPosition]);
  else a.flags = rec == kModeVelocity ? kFlagActualIsVelocity : rec == kModeForce ? kFlagForceMode : 0u;
  return a;
}

// The controller half of a general-path launch that does not change over the handle's life.
inline GenCtl gen_record(const cdpr_config_t& c, const KernelPlan& plan, const PidTerms pid[2], const GenLayout& lay, int rec) {
  GenCtl g;
  memset(&g, 0, sizeof g);
  g.mode = rec == kArgsPerRobot ? (int)kModePosition : rec;  // (per-robot handles: mode_arr decides)
  // JFC.cpp:72 compares the Joy axis (a float32) promoted to double with the double epsilon.  The kernels compare in float32: with the
  // largest float32 that is not above epsilon, t > g.eps holds for a float32 t exactly when (double)t > epsilon.  (float)epsilon
  // alone may round UP (0.001, 0.004): a target equal to it would then hold position where the reference runs the velocity Pid.
  g.eps = (float)c.velocity_epsilon;
  if ((double)g.eps > c.velocity_epsilon) g.eps = nextafterf(g.eps, -INFINITY);
  g.dt = (float)c.dt;
  g.lay = lay;
  const PidTerms &p0 = pid[0], &p1 = pid[1];
  g.pcas_max = std::max(p0.pcas, p1.pcas);
  g.dcas_max = std::max(p0.dcas, p1.dcas);
  g.nbuf0 = p0.nbuf, g.nbuf1 = p1.nbuf;
  g.hot = plan.gen_hot ? 1 : 0;
  const bool same_window = p0.nbuf == p1.nbuf && p0.degree == p1.degree;
  const bool clamps = p0.clamp32 && p1.clamp32 && (float)p0.imax >= (float)p0.imin && (float)p1.imax >= (float)p1.imin;
  g.simple_ok = (same_window && clamps && g.pcas_max == 0 && g.dcas_max == 0) ? 1 : 0;
  return g;
}

// A precision = 64 launch.  Per-robot handles: mode, Pid call count and so the Pid per lane - the velocity Pid in the primary fields,
// the position Pid in alt_*; HOLD handles: both Pids alive in the same places, the hold branch's parameters, the cascades' coefficients.
inline F64Args f64_record(const cdpr_config_t& c, const KernelPlan& plan, const PidTerms pid[2], int rec) {
  F64Args a;
  memset(&a, 0, sizeof a);
  fill_physics<double>(c, a);
  a.fk = plan.fk ? 1 : 0, a.td = plan.td ? 1 : 0;
  a.travel_stop = plan.tstop64 ? (int)c.travel_stop : 0;
  const bool pr = rec == kArgsPerRobot, vel = pr || rec == kModeVelocity;
  write_pid64(pid[vel || plan.hold64], a);
  if (pr || plan.hold64) write_alt64(pid[kPidPosition], a);
  if (plan.hold64) {
    write_hold64(pid, hold_win(plan), a);
    a.hold_eps = c.velocity_epsilon;
    a.hold_mode = pr ? (int)kModeVelocity : rec;
  }
  if (!pr) a.flags = vel ? kFlagActualIsVelocity : rec == kModeForce ? kFlagForceMode : 0u;
  return a;
}

inline LaunchArgs launch_args(const cdpr_config_t& c, const KernelPlan& plan, EnvFn env = process_env) {
  LaunchArgs L;
  L.pid[kPidPosition] = pid_terms(c.position_pid);
  L.pid[kPidVelocity] = pid_terms(c.velocity_pid);
  L.glay = GenLayout{0, 0, 0};
  if (plan.general)  // cables, the longest window of the two Pids, the deepest cascade
    L.glay = GenLayout{(int)c.n_cables, std::max(L.pid[0].nbuf, L.pid[1].nbuf), std::max(std::max(L.pid[0].pcas, L.pid[0].dcas), std::max(L.pid[1].pcas, L.pid[1].dcas))};
  if (plan.general) gen_tables(L.pid, L.glay.nb, L.ptab, L.gwtab);
  else if (plan.fp64) rotated_tables(L.pid, win64(plan), L.wtab64);
  else rotated_tables(L.pid, kWin, L.wtab);
  for (int rec = 0; rec < kArgsRecords; ++rec) {  // (every handle gets all three shapes: the ones its path never launches cost nothing)
    L.step[rec] = step_record(c, plan, L.pid, rec, env);
    L.gen[rec] = gen_record(c, plan, L.pid, L.glay, rec);
    L.f64[rec] = f64_record(c, plan, L.pid, rec);
  }
  return L;
}

// The bytes of what launch_args builds for `mode` (pointers null, tables appended): the record(s) a launch copies, then the path's
// uploaded tables.  cdpr_debug_launch_args, args_check.hip.
inline std::vector<unsigned char> launch_args_image(const LaunchArgs& L, const KernelPlan& plan, int mode) {
  std::vector<unsigned char> out;
  const auto put = [&out](const void* p, size_t bytes) { out.insert(out.end(), (const unsigned char*)p, (const unsigned char*)p + bytes); };
  const int rec = args_index(plan, mode);
  if (plan.fp64) put(&L.f64[rec], sizeof(F64Args));
  else put(&L.step[rec], sizeof(StepArgs));
  if (plan.general) put(&L.gen[rec], sizeof(GenCtl));
  put(L.wtab64.data(), L.wtab64.size() * sizeof(double));  // (a path has its own tables and no other's)
  put(L.wtab.data(), L.wtab.size() * sizeof(float));
  put(L.ptab.data(), L.ptab.size() * sizeof(float));
  put(L.gwtab.data(), L.gwtab.size() * sizeof(float));
  return out;
}

}  // namespace cdpr_host
