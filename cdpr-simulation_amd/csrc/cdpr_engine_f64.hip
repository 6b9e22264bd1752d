// cdpr_engine_f64.hip - host side of cdpr_config_t.precision = 64: the handle's set-up (build_f64), the fp64 step kernels' path of the
// launch chain (cdpr_step_kernel_f64.hpp), and the rollout by composition; both start from h->args.f64 (cdpr_launch_args.hpp: every
// constant of a launch, hold branch included, is made once by cdpr_create).  Reference paths as in cdpr_engine.hip.
#include "cdpr_engine_internal.hpp"

namespace cdpr {

// ---- cdpr_rollout_velocity on a precision = 64 handle (round 6), by composition: every (robot, sampled sequence) becomes a column
// of a scratch state (expand), every step of the horizon is ONE launch of the handle's own step kernel over those columns with the
// step's commands gathered into a Joy batch (cmd), and a third kernel adds |p(t_k+1) - p_ref|^2 to the trajectory's cost (cost).
// No rollout kernel of its own: the rollout in double is there for checking the fp32 one, not for throughput.
struct Roll64Args {
  const double* src;  // the handle's state rows
  double* dst;        // the trajectories' state rows
  uint32_t src_stride, dst_stride, rows, batch, samples;
  uint32_t zero_from;  // rows >= this are cleared in the copies (a Joy on jointVelocities in Position mode resets the velocity Pid,
                       // JFC.cpp:113-115); == rows: none
  // HOLD handles: that Pid has a record of its own per cable (f64_hold_row) - hold_zero_pid = 1 + the Pid whose records are cleared, 0: none
  uint32_t hold_base, hold_cable_rows, hold_pid_rows, hold_zero_pid;
  // per-robot handles: the robot's mode / call-count byte decides (a robot that is not in Velocity mode enters it: its - velocity - Pid
  // is reset, its count 0); every trajectory gets its own byte
  const uint8_t* meta_src;
  uint8_t* meta_dst;
};
static __global__ __launch_bounds__(256) void cdpr_roll64_expand_kernel(const Roll64Args a) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.batch * a.samples) return;
  const uint32_t b = t / a.samples;
  bool resets = true;  // (uniform handles: zero_from / hold_zero_pid already say whether the Joy resets the Pid)
  if (a.meta_src) {
    const uint32_t m = a.meta_src[b];
    resets = (m & kMetaModeMask) != kMetaVelocity;
    a.meta_dst[t] = (uint8_t)(resets ? kMetaVelocity : m);
  }
  for (uint32_t r = 0; r < a.rows; ++r) {
    bool zero = resets && r >= a.zero_from;
    if (resets && a.hold_zero_pid && r >= a.hold_base) {
      const uint32_t in_cable = (r - a.hold_base) % a.hold_cable_rows, first = 1u + (a.hold_zero_pid - 1u) * a.hold_pid_rows;
      zero = zero || (in_cable >= first && in_cable < first + a.hold_pid_rows);
    }
    a.dst[(size_t)r * a.dst_stride + t] = zero ? 0.0 : a.src[(size_t)r * a.src_stride + b];
  }
}
struct Roll64CmdArgs {
  const float* commands;  // float[B][H][S][n]
  float* out;             // float[B * S][n]: the Joy batch of step k
  uint32_t batch, samples, horizon, n, k;
};
static __global__ __launch_bounds__(256) void cdpr_roll64_cmd_kernel(const Roll64CmdArgs a) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.batch * a.samples * a.n) return;
  const uint32_t t = e / a.n, i = e - t * a.n, b = t / a.samples, s = t - b * a.samples;
  a.out[e] = a.commands[(((size_t)b * a.horizon + a.k) * a.samples + s) * a.n + i];
}
struct Roll64CostArgs {
  const double* state;  // the trajectories' state rows (rows 0..2: position)
  const float* ref;     // float[B][3]
  double* acc;          // double[B * S]
  float* out;           // float[B][S], written with the last step (nullptr before)
  uint32_t stride, batch, samples;
};
static __global__ __launch_bounds__(256) void cdpr_roll64_cost_kernel(const Roll64CostArgs a) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.batch * a.samples) return;
  const uint32_t b = t / a.samples;
  const double ex = a.state[t] - (double)a.ref[3 * b], ey = a.state[(size_t)a.stride + t] - (double)a.ref[3 * b + 1],
               ez = a.state[(size_t)2 * a.stride + t] - (double)a.ref[3 * b + 2];
  const double c = a.acc[t] + fma(ez, ez, fma(ey, ey, ex * ex));
  a.acc[t] = c;
  if (a.out) a.out[t] = (float)c;
}

}  // namespace cdpr

namespace cdpr_host {

// rows of an fp64 handle's state: platform, FK estimate, one Pid's rows per cable - and, hold branch live, both Pids' records
size_t state64_rows(const cdpr_engine* h) { return (size_t)f64_state_rows((int)h->n, win64(h->plan)) + (h->plan.hold64 ? (size_t)f64_hold_rows((int)h->n, hold_win(h->plan)) : 0); }

// cdpr_create's part of a precision = 64 handle: state and observables in double, the cable geometry, the two Pids' rotated weight
// tables for the ring of this handle's kernels (10, or 31 with windows of 12 .. 32 samples; launch_args made them), the debug rows
int build_f64(cdpr_engine* h) {
  const cdpr_config_t& cfg = h->cfg;
  const size_t row = (size_t)h->stride * sizeof(double);
  CREATE_TRY(h, "hipMalloc(state64)", h->d_state64.alloc(row * state64_rows(h)));
  CREATE_TRY(h, "hipMalloc(obs64)", h->d_obs64.alloc(row * f64_obs_rows((int)h->n)));
  std::vector<double> g((size_t)h->n * 7);
  for (uint32_t i = 0; i < h->n; ++i) {
    for (int k = 0; k < 3; ++k) {
      g[(size_t)i * 7 + k] = cfg.frame_anchor[i][k];
      g[(size_t)i * 7 + 3 + k] = cfg.platform_anchor[i][k];
    }
    g[(size_t)i * 7 + 6] = cfg.cable_ref_length[i];
  }
  if (int rc = upload_table(h, h->d_geom64, g.data(), g.size() * sizeof(double), "geom64")) return rc;
  if (int rc = upload_table(h, h->d_wtab64, h->args.wtab64.data(), h->args.wtab64.size() * sizeof(double), "wtab64")) return rc;
  if (h->dbg) CREATE_TRY(h, "hipMalloc(dbg64)", h->d_dbg64.alloc((size_t)h->batch * CDPR_PID_DEBUG_AXES * sizeof(double)));
  return CDPR_OK;
}

// fp64 handles: home state (platform at home, FK seed at home, controller rows zero), observables before the first publish
int upload_home64(cdpr_engine* h) {
  const size_t st = h->stride;
  std::vector<double> s(state64_rows(h) * st, 0.0), o((size_t)f64_obs_rows((int)h->n) * st, 0.0);
  for (uint32_t r = 0; r < h->stride; ++r)
    for (int c = 0; c < 7; ++c) {
      s[(size_t)(kF64Pose + c) * st + r] = h->cfg.home_pose[c];
      s[(size_t)(kF64StateFk + c) * st + r] = h->cfg.home_pose[c];
      o[(size_t)(kF64Pose + c) * st + r] = h->cfg.home_pose[c];
    }
  HIP_TRY(h, hipMemcpyAsync(h->d_state64, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_obs64, o.data(), o.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (h->d_dbg64) HIP_TRY(h, hipMemsetAsync(h->d_dbg64, 0, (size_t)h->batch * CDPR_PID_DEBUG_AXES * sizeof(double), h->stream));
  if (h->d_mode) HIP_TRY(h, hipMemsetAsync(h->d_mode, kModePosition, h->batch, h->stream));  // PLG.cpp:153-157 (call count 0)
  if (h->d_target) HIP_TRY(h, hipMemsetAsync(h->d_target, 0, (size_t)h->stride * h->n * sizeof(float), h->stream));
  for (int i = 0; i < 2; ++i)
    for (CmdChannel& c : h->cmd) HIP_TRY(h, hipMemsetAsync(c.d[i], 0, (size_t)h->stride * h->n * sizeof(float), h->stream));
  HIP_TRY(h, wait_stream(h));
  return CDPR_OK;
}

// precision = 64: the same host logic (commands are latched by run_steps before this is reached), the fp64 kernel
int run_steps_f64(cdpr_engine* h, int nsteps, int per_launch, bool reset_pid, void* record, const PlannedKernel& pk1, const PlannedKernel& pkk) {
  const uint32_t n = h->n;
  if (reset_pid && !h->plan.hold64) {  // Pid::reset (Pid.cpp:100-115): zero every controller row (hold branch live: the latch reset that Pid's own rows)
    h->pid_calls = 0;
    HIP_TRY(h, hipMemsetAsync(h->d_state64 + (size_t)kF64StateCtrl * h->stride, 0, (size_t)(win64(h->plan) + 1) * n * h->stride * sizeof(double), h->stream));
  }
  F64Args a = h->args.f64[args_index(h)];
  if (!h->plan.per_robot) a.cmd = h->cmd[cmd_kind_of_mode(h->mode)].latched();
  a.obs_step_stride = record ? (size_t)f64_obs_rows((int)n) * h->stride : 0;  // doubles per observable image
  // The routing: pk1 and pkk, planned_kernel's answers (cdpr_select.hpp) for a one-step and for a several-steps launch of this call
  // (run_steps made them in front of the latch).  One step per launch on FK + TD handles: estimator wave + controller wave
  // (cdpr_split_kernel_f64); up to one workgroup per CU its one-step launches beat the one-wave kernel's several-steps ones (14.4
  // against 20.8 us per step at one robot x 8, same bits): a fused update then runs as one-step launches
  if (pkk.id == KernelId::F64Split || pkk.id == KernelId::F64SplitHold) per_launch = 1;
  const uint32_t mode_flags = a.flags;
  return run_chain(h, nsteps, per_launch, record, h->d_obs64, [&](ChainStep& s) {
    a.nsteps = s.k;
    a.flags = mode_flags | s.first_flag;
    if (s.record) a.obs = static_cast<double*>(s.record);
    a.pid_calls = sat_pid_calls(h->pid_calls);
    a.ring_slot = ring_slot_of(h->step, win64(h->plan));
    a.step0 = (int)h->step;
    a.publish_mask = s.publish_mask;
    const PlannedKernel& pk = s.k == 1 ? pk1 : pkk;
    hipLaunchKernelGGL(f64_entry(pk), dim3(pk.grid(h->batch)), dim3(pk.block), 0, h->stream, a);
    h->last_kernel = pk;
    HIP_TRY(h, hipGetLastError());
    return (int)CDPR_OK;
  });
}

// Queue one rollout on the handle's stream: trajectories = batch * samples, reference positions and costs in
// DEVICE buffers.  Nothing is allocated, copied or synchronised here.
// The rollout of a precision = 64 handle (uniform modes; with the hold branch / cascades / cmd_limit 0 since the end of round 6): see Roll64Args above.
int rollout_enqueue_f64(cdpr_engine* h, int samples, int horizon, const float* d_commands, const float* d_ref, float* d_cost) {
  const uint32_t n = h->n;
  const uint64_t traj = (uint64_t)h->batch * (uint64_t)samples;
  const size_t cols = (size_t)((traj + 63u) & ~(uint64_t)63u);
  const uint32_t rows = (uint32_t)state64_rows(h);  // (hold branch live: both Pids' records of every cable travel with a trajectory)
  // (the four grow together; roll64_cols, the trajectories' row stride, never shrinks, so a buffer that failed to grow comes back at that size)
  const size_t cap = std::max(cols, h->roll64_cols);
  HIP_TRY(h, h->d_roll64.ensure(h, (size_t)rows * cap * sizeof(double)));
  HIP_TRY(h, h->d_roll64_acc.ensure(h, cap * sizeof(double)));
  HIP_TRY(h, h->d_roll64_cmd.ensure(h, cap * n * sizeof(float)));
  if (h->plan.per_robot) HIP_TRY(h, h->d_roll64_meta.ensure(h, cap));
  h->roll64_cols = cap;
  const bool pr = h->plan.per_robot;
  const bool reset = pr || h->mode != kModeVelocity;  // JFC.cpp:113-115: the copies start from a reset velocity Pid, the handle's rows stay (per-robot handles: per robot, from its meta byte)
  const uint32_t blocks = (uint32_t)((traj + 255u) / 256u);
  Roll64Args e{};
  e.src = h->d_state64, e.dst = h->d_roll64, e.src_stride = h->stride, e.dst_stride = (uint32_t)h->roll64_cols, e.rows = rows, e.batch = h->batch,
  e.samples = (uint32_t)samples, e.zero_from = (reset && !h->plan.hold64) ? (uint32_t)kF64StateCtrl : rows;
  if (h->plan.hold64 && reset) {  // ... there the velocity Pid's own record of every cable is what the Joy resets
    e.hold_base = (uint32_t)f64_state_rows((int)n), e.hold_cable_rows = (uint32_t)hold_cable_rows(hold_win(h->plan)), e.hold_pid_rows = (uint32_t)hold_pid_rows(hold_win(h->plan));
    e.hold_zero_pid = 2u;  // 1 + the Pid's index
  }
  if (pr) e.meta_src = h->d_mode, e.meta_dst = h->d_roll64_meta;
  hipLaunchKernelGGL(cdpr_roll64_expand_kernel, dim3(blocks), dim3(256), 0, h->stream, e);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemsetAsync(h->d_roll64_acc, 0, cols * sizeof(double), h->stream));
  F64Args a = h->args.f64[args_index(h->plan, kModeVelocity)];  // Velocity mode, whatever mode the handle is in (nothing is published: publish_mask = 0)
  a.state = h->d_roll64;
  a.dbg = nullptr;
  a.cmd = h->d_roll64_cmd;  // (per-robot handles: the trajectory's ACTIVE target row)
  if (pr) a.meta = h->d_roll64_meta;
  a.batch = (uint32_t)traj;
  a.stride = (uint32_t)h->roll64_cols;
  a.nsteps = 1;
  LaunchShape shape = launch_shape(h, horizon);  // the handle's one-wave kernel, rings in memory (planned_kernel's rollout rule)
  shape.rollout = true;
  const PlannedKernel pk = planned_kernel(h->plan, shape);
  const F64Kernel kern = f64_entry(pk);
  h->last_kernel = pk;
  const uint32_t mode_flags = a.flags;
  int calls = reset ? 0 : h->pid_calls;  // (uniform handles; per-robot handles count in the meta bytes)
  for (int k = 0; k < horizon; ++k) {
    Roll64CmdArgs c{};
    c.commands = d_commands, c.out = h->d_roll64_cmd, c.batch = h->batch, c.samples = (uint32_t)samples, c.horizon = (uint32_t)horizon, c.n = n, c.k = (uint32_t)k;
    hipLaunchKernelGGL(cdpr_roll64_cmd_kernel, dim3((uint32_t)((traj * n + 255u) / 256u)), dim3(256), 0, h->stream, c);
    const bool first_world = (steps_since_load(h) + (uint64_t)k) == 0;
    a.flags = mode_flags | (first_world ? kFlagFirstWorldStep : 0u);
    a.pid_calls = sat_pid_calls(calls);
    a.ring_slot = ring_slot_of(h->step + (uint64_t)k, win64(h->plan));
    a.step0 = (int)(h->step + (uint64_t)k);
    hipLaunchKernelGGL(kern, dim3(pk.grid(traj)), dim3(pk.block), 0, h->stream, a);
    calls = sat_pid_calls(calls + (first_world ? 0 : 1));
    Roll64CostArgs q{};
    q.state = h->d_roll64, q.ref = d_ref, q.acc = h->d_roll64_acc, q.out = (k == horizon - 1) ? d_cost : nullptr, q.stride = (uint32_t)h->roll64_cols,
    q.batch = h->batch, q.samples = (uint32_t)samples;
    hipLaunchKernelGGL(cdpr_roll64_cost_kernel, dim3(blocks), dim3(256), 0, h->stream, q);
    HIP_TRY(h, hipGetLastError());
    h->launches += 1;
  }
  return CDPR_OK;
}

}  // namespace cdpr_host
