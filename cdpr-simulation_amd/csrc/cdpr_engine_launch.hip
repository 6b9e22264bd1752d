// cdpr_engine_launch.hip - what turns "advance n world steps" into launches: the latch of the pending commands, the clock of the chain
// the three paths share (run_chain, cdpr_engine_internal.hpp: publish_mask, advance_clock), the register-resident path's launches with their hipGraph replay
// (run_steps), the general controller path's (run_steps_general; precision = 64: run_steps_f64, cdpr_engine_f64.hip), and command
// schedules (scheduled_update).  Every launch copies the handle's argument record of the current mode (h->args, cdpr_launch_args.hpp) and
// assigns the per-launch fields listed at the top of that header.  Reference paths as in cdpr_engine.hip.
#include "cdpr_engine_internal.hpp"

namespace cdpr {

// Per-robot command arrival (latch_robot, cdpr_robot_records.hpp): one thread per robot, one kernel per record layout
template <typename View>
CDPR_DEV void latch_thread(const LatchWho& who, const View& v) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (latch_wanted(who, v.batch, r)) latch_robot(who, v, r);
}
static __global__ __launch_bounds__(256) void cdpr_latch_fast_kernel(const LatchWho who, const FastRecords v) { latch_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_gen_latch_kernel(const LatchWho who, const GenRecords v) { latch_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_latch_f64_kernel(const LatchWho who, const F64Records v) { latch_thread(who, v); }

// ... and the general path's hot rows back into the H slots, every robot's
static __global__ __launch_bounds__(256) void cdpr_gen_flush_hot_kernel(const int nbuf, const GenRecords v) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < v.batch) flush_hot_robot(v, nbuf, r);
}

// cdpr_update_scheduled_kind served as a chain of launches: one thread waits for the mailbox word of the next batch in front
// of the batch's latch (what sched_wait does inside a launch that carries the schedule itself).
static __global__ void cdpr_mailbox_wait_kernel(const uint32_t* word, uint32_t* fault) { mailbox_wait(word, fault); }

}  // namespace cdpr

namespace cdpr_host {

double sim_time(uint64_t step, double dt) {
  // gazebo::common::Time keeps integer sec + nsec; Double() = sec + nsec * 1e-9 [EXT]
  const int64_t dt_ns = (int64_t)std::llround(dt * 1e9);
  const int64_t now_ns = (int64_t)step * dt_ns;
  return (double)(now_ns / 1000000000LL) + (double)(now_ns % 1000000000LL) * 1e-9;
}

// Which of the next k world steps publish (bit j: world step h->step + j; launches of more than 64 steps publish by flag),
// PLG.cpp:236-242: strict '>' against the last published stamp, which moves on with every step that does - `last` is where it
// stands after the k steps.  publish_period == 0: every step but world step 0 (whose stamp is not above the initial 0).
uint64_t publish_mask(const cdpr_engine* h, int k, double& last) {
  uint64_t mask = 0;
  last = h->prev_publish;
  if (h->cfg.publish_period == 0.0) {
    if (k > 0 && steps_since_load(h) + (uint64_t)k > 1) last = sim_time(h->step + (uint64_t)k - 1, h->cfg.dt);
    mask = (k >= 64) ? ~0ull : ((1ull << k) - 1ull);
    return steps_since_load(h) == 0 ? (mask & ~1ull) : mask;
  }
  for (int j = 0; j < k; ++j) {
    const double now = sim_time(h->step + (uint64_t)j, h->cfg.dt);
    if ((now - last) > h->cfg.publish_period) {
      last = now;
      if (j < 64) mask |= (1ull << j);
    }
  }
  return mask;
}

// The handle's clock after k world steps were queued in `launches` launches - every path, eager or replayed, ends here.  The publish
// stamp follows the rule above.  Pid::update calls since the last Pid reset: none in Force mode, none at world step 0 (the plugin's
// first update only stores the joint positions), and the count saturates at kCallSat (the kernels ask "0?" and ">= nbuf?"); the
// general path keeps its counts on the device, in the controller records.
void advance_clock(cdpr_engine* h, int k, int launches) {
  (void)publish_mask(h, k, h->prev_publish);
  if (!h->plan.general && h->mode != kModeForce) h->pid_calls = sat_pid_calls(h->pid_calls + k - (steps_since_load(h) == 0 ? 1 : 0));
  h->step += (uint64_t)k;
  h->launches += (uint64_t)launches;
}

// Weights of ring position `slot`, copied into a launch's arguments (see StepArgs::wrow).
static void set_weight_row(const cdpr_engine* h, StepArgs& a, int slot) {
  // (per-robot handles: both Pids share one window, so the velocity Pid's table serves every lane)
  const int table = (h->plan.per_robot || h->mode == kModeVelocity) ? 0 : kWin;  // first row of [velocity | position]
  memcpy(a.wrow, &h->args.wtab[(size_t)(table + slot) * (kWin + 2)], sizeof a.wrow);
}

// The kernel a launch uses: the routing is planned_kernel's (cdpr_select.hpp: a pure function of the handle's plan and the
// launch's shape, the same one cdpr_plan_kernel answers from without a GPU).  Its answer names one instantiation completely: a
// launch site reads planned_kernel -> step_entry / gen_entry / f64_entry (cdpr_kernels.hpp) -> launch, grid and block from the answer.
LaunchShape launch_shape(const cdpr_engine* h, int k, bool steady, const Schedule* sched) {
  LaunchShape s;
  s.steps = k;
  s.first_world = steps_since_load(h) == 0;
  s.scheduled = sched != nullptr;
  s.steady = steady;
  s.vel = h->mode == kModeVelocity;
  if (h->plan.fp64) {  // the per-call A/B overrides (read per call: A/B in one process)
    const auto env_int = [](const char* key) { const char* v = std::getenv(key); return v ? atoi(v) : -1; };
    s.f64_ring_lds = env_int("CDPR_F64_RING_LDS");  // the rings in LDS (64 KiB per wave at n = 8: two waves per CU) while the batch leaves CUs to spare
    s.f64_jcache = env_int("CDPR_F64_JCACHE");      // ... and the structure-matrix rows too (112 KiB: one wave per CU) up to one workgroup per CU
    s.f64_split = env_int("CDPR_F64_SPLIT");        // 0 never, 1 the LDS-cached build, 2 the lean build whatever the batch
  }
  return s;
}
// A kernel without an instantiation is refused, not launched (`missing`: missing_entry's answer, id None where nothing is missing).
// Which kernels a handle's launches can take is a function of its plan alone: cdpr_create asks for every launch shape there is
// (build_handle) and refuses the handle.  Only precision = 64 reads overrides per call: run_steps asks again for that call's two
// kernels, in front of the latch.  No configuration gets here today.
int refuse_missing(cdpr_engine* h, const PlannedKernel& missing) {
  if (missing.id == KernelId::None) return CDPR_OK;
  h->err = "internal: no instantiation for " + planned_kernel_name(missing);
  return CDPR_ERR_UNSUPPORTED;
}
// May a launch of k > 1 world steps with the arguments `a` (flags, pid_calls, pointers set) run on cdpr_pair_stream_kernel?
// That kernel has no branch for anything but the steady state of a plain handle (cdpr_step_kernel_pair.hpp): every
// condition below is one the general several-steps kernel tests per step instead (LaunchShape::steady).  CDPR_PAIR_STREAM=0: never (A/B).
static bool pair_stream_steady(const cdpr_engine* h, const StepArgs& a, const Schedule* sched) {
  return steps_since_load(h) != 0 && h->mode != kModeForce && a.pid_calls >= a.nbuf && h->cfg.publish_period == 0.0 && !a.dbg && !a.travel_on &&
         !(a.vel_limit > 0.f) && !a.unilateral && a.effort >= 0.f && a.clamp_cmd && !(sched && sched->ready);
}
// Can the handle's role-split launches ever take the steady-state kernel (cdpr_split_steady_kernel<N, VEL>, cdpr_onestep_kernel.hpp)?  What
// does not change over the handle's life: a uniform handle, every step published, and the estimator wave's contract - its Newton stage is
// four iterations written out without a convergence test, which is the generic loop exactly for a tolerance of 0 and 4 iterations.
// CDPR_SPLIT_STEADY=0: never (A/B, tests).
static bool split_steady_handle(const cdpr_engine* h) {
  return h->split_steady && !h->plan.per_robot && h->cfg.publish_period == 0.0 && h->cfg.fk_tolerance == 0.0 && h->cfg.fk_max_iterations == 4;
}
// May a launch of the role-split kernel with the arguments `a` take it (LaunchShape::split_steady; planned_kernel asks it of that kernel
// only)?  The steady kernel has no code for anything the generic one tests per launch and these facts decide: such a handle in Velocity
// or Position mode, past world step 0, the derivative window full, no `pid` topic, no travel flags.  Same bits either way (tested).
static bool split_steady_launch(const cdpr_engine* h, const StepArgs& a) {
  return split_steady_handle(h) && steps_since_load(h) != 0 && h->mode != kModeForce && a.pid_calls != 0 && a.pid_calls >= a.nbuf && !a.dbg && !a.travel_on;
}

// What the register-resident path adds to the record of the handle's mode for a whole call: the latched command rows (per-robot handles:
// the active target rows are bound in the record), a trajectory record's stride; with a schedule (a whole one in one launch;
// publish_period == 0, every step but world step 0 is published) its batches, mailbox and status word.
static StepArgs fast_path_args(const cdpr_engine* h, const void* record, const Schedule* sched) {
  StepArgs a = h->args.step[args_index(h)];
  if (!h->plan.per_robot) a.cmd = h->cmd[cmd_kind_of_mode(h->mode)].latched();  // position: all zeros until the first jointPositions message: target 0 (PLG.cpp:153-157)
  a.obs_step_stride = record ? (size_t)h->n_obs * h->stride : 0;
  if (sched) {
    a.flags |= kFlagPublishAll;
    a.sched_refresh = sched->refresh;
    a.sched_stride = (size_t)h->batch * h->n;
    a.sched_ready = sched->ready;
    a.fault = sched->fault;
  }
  return a;
}

// cdpr_create pays the cold costs of the handle's one-step kernel (the runtime loads a kernel's code object and sets up
// its argument buffers on the FIRST launch: measured ~1 ms), not the first cdpr_update: one launch of exactly that kernel
// over one workgroup of home-state robots in a scratch buffer, which is then freed.  The handle's own state is not touched.
int warm_first_launch(cdpr_engine* h) {
  if (h->plan.general || h->plan.fp64) return CDPR_OK;
  if (const char* w = std::getenv("CDPR_NO_WARM_LAUNCH"))
    if (w[0] == '1') return CDPR_OK;
  const PlannedKernel pk = planned_kernel(h->plan, launch_shape(h, 1));
  const uint32_t rows = 64;
  const std::vector<float4> s = home_state(h, rows);
  DevBuf st, ob, cm, mt;
  HIP_TRY(h, mt.alloc(rows));
  HIP_TRY(h, hipMemsetAsync(mt.p, (int)(kMetaPosition | (20u << kMetaCallShift)), rows, h->stream));
  HIP_TRY(h, st.alloc(s.size() * sizeof(float4)));
  HIP_TRY(h, ob.alloc((size_t)h->n_obs * rows * sizeof(float4)));
  HIP_TRY(h, cm.alloc((size_t)rows * h->n * sizeof(float)));
  HIP_TRY(h, hipMemcpyAsync(st.p, s.data(), s.size() * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(cm.p, 0, (size_t)rows * h->n * sizeof(float), h->stream));
  StepArgs a = h->args.step[args_index(h)];  // Position mode, where a fresh handle stands, over the scratch robots
  a.state = st.as<float4>(), a.obs = ob.as<float4>(), a.cmd = cm.as<float>(), a.meta = mt.as<uint8_t>(), a.dbg = nullptr;
  a.batch = pk.robots_per_block, a.stride = rows;
  a.nsteps = 1;
  a.publish_mask = 1ull;
  a.pid_calls = kCallSat;  // steady state: every branch of the step is taken, as in the launches that follow
  a.ring_slot = 0;
  set_weight_row(h, a, 0);
  hipLaunchKernelGGL(step_entry(pk), dim3(1), dim3(pk.block), 0, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  // ... and of the role-split kernel's steady-state instantiations, which the launches take from the step on that fills the window
  // (split_steady_launch): both modes' - a Joy of the other kind may arrive at any step (the mode is the instantiation's, the gains do
  // not matter to a launch whose results are dropped)
  for (const bool vel : {false, true}) {
    LaunchShape shape = launch_shape(h, 1);
    shape.split_steady = split_steady_handle(h), shape.vel = vel;
    const PlannedKernel steady = planned_kernel(h->plan, shape);
    if (!steady.steady) break;
    hipLaunchKernelGGL(step_entry(steady), dim3(1), dim3(steady.block), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, wait_stream(h));
  return CDPR_OK;
}

// One step-kernel launch over the whole batch, or (h->plan.chunk) the same launch cut into contiguous blocks of robots issued
// back to back on the handle's stream: every pointer that is indexed by robot moves to the block's first robot, the row
// stride stays.  Robots are independent, so the results are bit-identical to the single launch (tested).  Returns the launches queued.
static int launch_step(cdpr_engine* h, StepKernel kern, const PlannedKernel& pk, const StepArgs& a, uint32_t max_grid = 0) {
  const uint32_t B = a.batch;
  const uint32_t chunk = (h->plan.chunk && B > h->plan.chunk) ? h->plan.chunk : B;
  const uint32_t pieces = (B + chunk - 1u) / chunk;
  const uint32_t each = (((B + pieces - 1u) / pieces) + 63u) & ~63u;  // balanced, whole wavefronts
  int launches = 0;
  for (uint32_t first = 0; first < B; first += each, ++launches) {
    StepArgs c = a;
    c.batch = std::min(each, B - first);
    c.state = a.state + first;
    c.obs = a.obs + first;
    if (a.cmd) c.cmd = a.cmd + (size_t)first * h->n;
    if (a.dbg) c.dbg = a.dbg + (size_t)first * CDPR_PID_DEBUG_AXES;
    if (a.meta) c.meta = a.meta + first;
    uint32_t grid = pk.grid(c.batch);
    if (max_grid && grid > max_grid) grid = max_grid;  // persistent kernel: the waves walk over the blocks
    hipLaunchKernelGGL(kern, dim3(grid), dim3(pk.block), 0, h->stream, c);
  }
  return launches;
}

// the general path's hot rows back into the H slots (cdpr_gen_flush_hot_kernel) before a Pid's records are reset or latched over
static void flush_hot(cdpr_engine* h) {
  if (!h->d_rec || !h->plan.gen_hot) return;
  hipLaunchKernelGGL(cdpr_gen_flush_hot_kernel, robot_grid(h), dim3(kRobotBlock), 0, h->stream, std::max(h->args.pid[kPidPosition].nbuf, 1), gen_records(h));
}

// Pid::reset of one Pid of every cable (general path): its slots, its rows
static hipError_t reset_block(cdpr_engine* h, int which) {
  const GenLayout& L = h->args.glay;
  flush_hot(h);
  hipError_t e1 = hipMemsetAsync(h->d_rec + (size_t)L.block_a(which, 0) * h->stride * 4, 0, (size_t)L.pid_slots() * h->stride * 16, h->stream);
  if (e1 != hipSuccess || L.pid_rows() == 0) return e1;
  return hipMemsetAsync(h->d_rec + ((size_t)L.slots() * 4 + (size_t)L.block_b(which, 0)) * h->stride, 0, (size_t)L.pid_rows() * h->stride * 4, h->stream);
}

// precision = 64 with the hold branch: Pid::reset of one Pid of every cable (its rows behind the state)
static hipError_t reset_block64(cdpr_engine* h, int which) {
  for (uint32_t i = 0; i < h->n; ++i) {
    hipError_t e1 = hipMemsetAsync(h->d_state64 + (size_t)f64_hold_row((int)h->n, (int)i, which, hold_win(h->plan)) * h->stride, 0, (size_t)hold_pid_rows(hold_win(h->plan)) * h->stride * sizeof(double),
                                   h->stream);
    if (e1 != hipSuccess) return e1;
  }
  return hipSuccess;
}

// Per-robot handles: every robot has its own mode, so a command of `kind` (masked or not) is latched on the device, robot by
// robot, by the latch kernel of the handle's record layout.  (The general path's latch zeroes a Pid's records for many robots at
// once: its hot rows are flushed first.  Nothing is drained: what the latch reads has passed ready_wait, latch_pending.)
static int latch_per_robot(cdpr_engine* h, int kind, const float* pending, const uint8_t* mask) {
  const CmdKind& K = kCmdKind[kind];
  if (h->plan.general) flush_hot(h);
  return launch_per_robot(h, LatchWho{mask, pending, (uint32_t)kind, K.meta, K.reset_pid}, cdpr_latch_fast_kernel, cdpr_gen_latch_kernel, cdpr_latch_f64_kernel, false);
}

// PLG.cpp:206-219: an update starts by latching the pending commands, velocity first, then position; force after the two
// Joy topics ([NEW] ordering: the reference has no force callback).  `reset_pid`: the mode change of a uniform handle asks
// the launches that follow to zero their single Pid record (register-resident path, precision = 64 without the hold branch).
static int latch_pending(cdpr_engine* h, bool& reset_pid) {
  for (CmdChannel& c : h->cmd) {
    if (c.pending && c.ready_wait) {  // a host Joy batch is (or was) on its way on the copy stream
      HIP_TRY(h, hipStreamWaitEvent(h->stream, c.ready_wait, 0));
      c.ready_wait = nullptr;
    }
  }
  bool touched[kCmdKinds] = {false, false, false};  // the engine's own pending buffer was read (latch kernel) or swapped
  for (int k = 0; k < kCmdKinds; ++k) {
    CmdChannel& c = h->cmd[k];
    if (!c.pending) continue;
    const CmdKind& K = kCmdKind[k];
    if (h->plan.per_robot) {
      // (a batch of a device-resident schedule, cdpr_update_scheduled_kind, is latched from the caller's buffers in place)
      const bool in_place = c.sched_rows != nullptr;
      if (int rc = latch_per_robot(h, k, in_place ? c.sched_rows : c.d[1].p, in_place ? c.sched_mask : (c.masked ? c.d_mask.p : nullptr))) return rc;
      touched[k] = !in_place;
    } else {
      if (c.ext[1]) {  // bound caller buffer: latched by pointer, nothing copied
        c.ext[0] = c.ext[1];
        c.ext[1] = nullptr;
      } else {
        c.d[0].swap(c.d[1]);
        c.ext[0] = nullptr;
        touched[k] = true;  // what is pending now was the latched buffer of the launches queued so far
      }
      if (K.reset_pid >= 0) {  // entering a mode resets its Pid (fast path: the single record now belongs to that Pid)
        reset_pid = (h->mode != K.mode);
        if (h->plan.general && reset_pid) HIP_TRY(h, reset_block(h, K.reset_pid));
        if (h->plan.hold64 && reset_pid) HIP_TRY(h, reset_block64(h, K.reset_pid));
      }
      h->mode = K.mode;
    }
    c.pending = c.masked = false;
    c.have = true;
  }
  for (CmdChannel& c : h->cmd) c.sched_rows = nullptr;
  // What is now the PENDING buffer of a touched kind was last used by the work queued on the compute stream so far: the next
  // host batch of that kind, which travels on the copy stream, may overwrite it only once that work is through.  The event is
  // recorded on EVERY such latch once a copy stream exists, however the latched command itself arrived (host, _device or
  // masked): a stale event from an earlier host batch would let the copy run into launches that still read the buffer.  Bound
  // commands swap nothing and handles that never saw a host batch have no copy stream: no event, no device time.
  for (int k = 0; k < kCmdKinds; ++k) {
    CmdChannel& c = h->cmd[k];
    if (!touched[k] || !h->copy_stream) continue;
    if (!c.free_ev) HIP_TRY(h, hipEventCreateWithFlags(&c.free_ev, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(c.free_ev, h->stream));
    c.free_ev_set = true;
  }
  return CDPR_OK;
}

// General controller path: ONE launch per `per_launch` world steps (cdpr_general_step.hpp); with `record`, the observable
// image of step j of the call goes to record + j * n_obs * stride.
static int run_steps_general(cdpr_engine* h, int nsteps, int per_launch, void* record) {
  StepArgs a = h->args.step[args_index(h)];  // (run_steps has asked general_clock_check: world-step stamps are int32 in the controller records)
  a.obs_step_stride = record ? (size_t)h->n_obs * h->stride : 0;
  GenCtl g = general_ctl(h);
  // where the role-split one-step kernel serves the handle, its launches beat the one-wave kernel's multi-step ones
  // (16 384 x 8: 9.2 against 13.7 us per step, 32 768: 10.1 against 21.6; same bits): fused updates and the trajectory
  // record then run as one-step launches
  if (h->plan.gen_split || h->plan.gen_lean) per_launch = 1;  // (likewise where the lean kernel + one-wave kernel pair steps the handle)
  return run_chain(h, nsteps, per_launch, record, h->d_obs, [&](ChainStep& s) {
    // one step per launch on FK + TD handles up to two workgroups per CU: the role-split form (cdpr_general_split.hpp), beyond: the
    // lean role-split kernel (two waves per SIMD; the rare controller paths by call) - planned_kernel, cdpr_select.hpp
    const PlannedKernel pk = planned_kernel(h->plan, launch_shape(h, s.k));
    h->last_kernel = pk;
    a.nsteps = s.k;
    a.flags = s.first_flag;
    g.now_step = (int)h->step;
    if (s.record) a.obs = static_cast<float4*>(s.record);
    a.publish_mask = s.publish_mask;
    hipLaunchKernelGGL(gen_entry(pk), dim3(pk.grid(h->batch)), dim3(pk.block), 0, h->stream, a, g);
    HIP_TRY(h, hipGetLastError());
    return (int)CDPR_OK;
  });
}

// Launches per captured graph = one ring period: a chain ends on the ring slot it started from.  (Ten, not more: a caller that refreshes
// its Joy batch every 10 steps - bench.py, the reference's 100 Hz publishers against the 1 kHz world - hands over 10 steps per call.)
constexpr int kGraphChunk = 10;

int run_steps(cdpr_engine* h, int nsteps, int per_launch, void* record, const Schedule* sched) {
  if (!h) return CDPR_ERR_INVALID;
  if (nsteps < 0 || per_launch < 1 || (per_launch > 64 && !sched)) {
    h->err = "nsteps must be >= 0 and steps_per_launch in 1..64";
    return CDPR_ERR_INVALID;
  }
  if (nsteps == 0) return CDPR_OK;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;

  if (int rc = general_clock_check(h, (uint64_t)nsteps)) return rc;  // (in front of the latch: a refused update leaves pending commands pending)
  PlannedKernel f64_kernels[2];  // precision = 64: the kernels of this call's one-step and several-steps launches (its overrides are read per call)
  if (h->plan.fp64)
    for (int i = 0; i < 2; ++i) {
      f64_kernels[i] = planned_kernel(h->plan, launch_shape(h, i + 1));
      if (!f64_entry(f64_kernels[i])) return refuse_missing(h, f64_kernels[i]);
    }
  bool reset_pid = false;
  if (int rc = latch_pending(h, reset_pid)) return rc;
  if (h->plan.general) return run_steps_general(h, nsteps, per_launch, record);
  if (h->plan.fp64) return run_steps_f64(h, nsteps, per_launch, reset_pid, record, f64_kernels[0], f64_kernels[1]);

  if (reset_pid) {  // Pid::reset (Pid.cpp:100-115): zero every controller record; rare, so done outside the step kernel
    h->pid_calls = 0;
    const int P = plat_slots(h->plan.fk);
    HIP_TRY(h, hipMemsetAsync(h->d_state + (size_t)P * h->stride, 0, (size_t)ctrl_slots((int)h->n) * h->stride * sizeof(float4), h->stream));
  }
  StepArgs a = fast_path_args(h, record, sched);
  const uint32_t mode_flags = a.flags;

  return run_chain(h, nsteps, per_launch, record, h->d_obs, [&](ChainStep& s) {
    const int k = s.k;
    a.nsteps = k;
    a.flags = mode_flags | s.first_flag;
    // the kernel uses calls != 0 and calls >= nbuf (<= 11): the count saturates, and the ring position follows the world
    // step, so steady-state launch sequences repeat with period 10
    a.pid_calls = sat_pid_calls(h->pid_calls);
    a.ring_slot = ring_slot_of(h->step);
    // a launch over a command schedule always runs on the several-steps kernel, even for one step: only that one reads the
    // schedule, its mailbox and kFlagPublishAll
    LaunchShape shape = launch_shape(h, sched ? std::max(k, 2) : k, pair_stream_steady(h, a, sched), sched);
    shape.split_steady = split_steady_launch(h, a);
    const PlannedKernel pk = planned_kernel(h->plan, shape);
    const StepKernel kern = step_entry(pk);
    h->last_kernel = pk;
    // steady state of a plain lane-pair handle: the branch-free several-steps kernel, which reads the weights by AGE from row 0
    const bool stream = pk.id == KernelId::PairStream;
    set_weight_row(h, a, stream ? 0 : a.ring_slot);
    if (s.record) a.obs = static_cast<float4*>(s.record);
    a.publish_mask = sched ? 0 : s.publish_mask;

    // Steady state (every step published, derivative window full, not t = 0): the next launches are
    // byte-identical, so replay them from a captured hipGraph instead of paying a host launch each.
    // (measured on MI355X: 3.57 -> 3.41 us/step at 4 096 x 4 cables; at 65 536 x 8 cables the 15 us kernels already
    // hide the host launch and the replay's fixed cost makes it 2 % slower, so only small batches use it)
    // (the ring position advances with every step, so a captured chain is only valid from the position it was captured at:
    //  part of the cache key; the call count must be saturated (per-robot handles keep theirs on the device))
    const bool steady = !record && !sched && h->use_graphs && (size_t)h->batch * h->n <= 131072u && !s.first_flag &&
                        (h->plan.per_robot || a.pid_calls == kCallSat || h->mode == kModeForce) && h->cfg.publish_period == 0.0 && s.left >= kGraphChunk * k;
    if (steady) {
      const GraphKey key{(void*)kern, a.cmd, k, a.ring_slot, a.flags};
      hipGraphExec_t exec = h->graphs.find(key);
      if (!exec)
        exec = h->graphs.capture(h->stream, key, [&] {
          bool launched = true;
          for (int j = 0; j < kGraphChunk; ++j) {
            StepArgs aj = a;  // each node carries its own ring position
            aj.ring_slot = (a.ring_slot + j * k) % kWin;
            set_weight_row(h, aj, stream ? 0 : aj.ring_slot);
            hipLaunchKernelGGL(kern, dim3(pk.grid(h->batch)), dim3(pk.block), 0, h->stream, aj);
            launched = launched && (hipGetLastError() == hipSuccess);
          }
          return launched;
        });
      if (exec) {
        HIP_TRY(h, hipGraphLaunch(exec, h->stream));
        s.used = kGraphChunk * k, s.launches = kGraphChunk;
        return (int)CDPR_OK;
      }
      h->use_graphs = false;  // ... and this chunk, like every later one, is launched eagerly
    }
    s.launches = launch_step(h, kern, pk, a, pk.persist ? h->persist_grid : 0u);
    HIP_TRY(h, hipGetLastError());
    return (int)CDPR_OK;
  });
}

// A command schedule resident in HBM, any kind of command, any handle.  Semantics: for j = 0 ..: the callback of `kind`
// with batch j (for the robots of mask j), then refresh_steps x update().  Two forms serve it:
//   * in the launch: uniform-mode handles on the register-resident path with one or two lanes per robot run the whole
//     schedule in ONE launch of the several-steps kernel (the lanes read batch j at step j * refresh_steps themselves;
//     state, windows and integrals stay on chip);
//   * as a chain: every other handle (general controller path, per-robot modes with or without masks, precision = 64,
//     one lane per cable) latches batch j from the caller's buffers in place and queues its steps, batch after batch,
//     without a host round trip; a mailbox is honoured by a one-thread wait kernel in front of the batch's latch.
// A command of another kind pending at the call is latched with batch 0 in update()'s usual order (velocity, position,
// force): batch 0 then goes the chain's way, so that a mode change between batch 0 and batch 1 is what the call sequence
// would do (the schedule's rows must never be read as targets of another mode).
int scheduled_update(cdpr_engine* h, uint32_t kind, int nsteps, int refresh_steps, const float* d_commands, const uint32_t* d_ready, const uint8_t* d_masks,
                     void* d_record, size_t record_bytes) {
  if (kind > 2u) {
    h->err = "cdpr_update_scheduled_kind: kind must be CDPR_COMMAND_VELOCITY, _POSITION or _FORCE";
    return CDPR_ERR_INVALID;
  }
  if (nsteps < 0 || refresh_steps < 1 || !d_commands) {
    h->err = "cdpr_update_scheduled: nsteps >= 0, refresh_steps >= 1 and the command schedule are required";
    return CDPR_ERR_INVALID;
  }
  if (d_masks && !h->plan.per_robot) {
    h->err = "cdpr_update_scheduled_kind: robot masks need a handle created with per_robot_commands = 1";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (h->cfg.publish_period != 0.0 && d_record) {
    h->err = "cdpr_update_scheduled: a trajectory record needs publish_period == 0 (every step published)";
    return CDPR_ERR_UNSUPPORTED;
  }
  const size_t image = image_bytes(h);
  if (d_record && record_bytes < image * (size_t)nsteps) {
    h->err = "cdpr_update_scheduled: record buffer smaller than nsteps observable images";
    return CDPR_ERR_INVALID;
  }
  if (nsteps == 0) return CDPR_OK;
  if (int rc = general_clock_check(h, (uint64_t)nsteps)) return rc;  // (the whole schedule: no batch is staged, latched or stepped)
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (d_ready && !h->h_fault) {  // the status word a mailbox that never delivers is reported through
    HIP_TRY(h, h->h_fault.alloc(sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    *h->h_fault = 0u;
    HIP_TRY(h, hipHostGetDevicePointer((void**)&h->d_fault, h->h_fault, 0));
  }
  auto record_at = [&](int done) -> void* { return d_record ? static_cast<char*>(d_record) + (size_t)done * image : nullptr; };
  const size_t batch_floats = (size_t)h->batch * h->n;
  CmdChannel& c = h->cmd[kind];
  const int nbatches = (nsteps + refresh_steps - 1) / refresh_steps;
  // batch j becomes the pending command of `kind`, in place
  auto stage_batch = [&](int j) {
    const float* rows = d_commands + (size_t)j * batch_floats;
    if (h->plan.per_robot) {
      c.sched_rows = rows;
      c.sched_mask = d_masks ? d_masks + (size_t)j * h->batch : nullptr;
    } else {
      c.ext[1] = rows;
    }
    c.pending = true;
    c.masked = false;
  };
  // Per-robot handles: a command of the SAME kind still pending at the call (cdpr_set_*_command[_masked] without an update since)
  // would have to reach its robots before batch 0 reaches batch 0's - B independent plugins each keep the last message that
  // reached THEM.  Staging batch 0 would overwrite it silently: refused, the caller latches it with cdpr_update first
  // or leaves it out.  (Uniform handles: the later message of a kind replaces the earlier one, as in the plugin, PLG.cpp:67-83.)
  if (h->plan.per_robot && c.pending) {
    h->err = "cdpr_update_scheduled_kind: a command of the same kind is still pending on this per-robot handle; step it in with cdpr_update first";
    return CDPR_ERR_INVALID;
  }
  // whatever way this function is left, nothing of the caller's schedule stays staged in the handle: an error return must not
  // leave `pending` set on pointers the caller may free
  struct Unstage {
    cdpr_engine* h; CmdChannel& c; bool ok = false;
    ~Unstage() {
      c.sched_rows = nullptr;
      c.sched_mask = nullptr;
      if (!ok) {  // an error in between: drop the batch that was staged but not latched
        if (c.pending && (h->plan.per_robot || c.ext[1])) c.pending = false;
        c.ext[1] = nullptr;
      }
    }
  } unstage{h, c};
  const bool in_launch = !(h->plan.general || h->plan.fp64 || h->plan.per_robot || h->plan.lane_cable) && h->cfg.publish_period == 0.0;
  bool others = false;
  for (uint32_t k = 0; k < (uint32_t)kCmdKinds; ++k) others = others || (k != kind && h->cmd[k].pending);
  int j = 0, done = 0;
  // ---- the chain: every batch of a handle the launch form does not serve; batch 0 where another command is pending
  const int chain_spl = ((size_t)h->batch * h->n <= 131072u) ? std::min(refresh_steps, 64) : 1;  // small batches: the hold in one launch
  while (j < nbatches && (!in_launch || (j == 0 && others))) {
    if (d_ready) {
      hipLaunchKernelGGL(cdpr_mailbox_wait_kernel, dim3(1), dim3(1), 0, h->stream, d_ready + j, h->d_fault);
      HIP_TRY(h, hipGetLastError());
    }
    stage_batch(j);
    const int k = std::min(refresh_steps, nsteps - done);
    if (int rc = run_steps(h, k, chain_spl, record_at(done))) return rc;
    done += k;
    ++j;
  }
  while (j < nbatches) {
    // ---- the rest in one launch: batch j is latched as any command of its kind is (entering the mode resets its Pid,
    //      JFC.cpp:101-103,113-115), the later ones are read by the kernel.  Lane-pair handles whose derivative windows are not
    //      full yet (world step 0, a mode just entered) take the batches that fill them in a launch of their own: from there on
    //      the launch qualifies for the steady-state kernel (pair_stream_ok), which has no branch for a filling window.
    stage_batch(j);
    const Schedule sched{refresh_steps, d_ready ? d_ready + j : nullptr, h->d_fault};
    int rest = nsteps - done;
    if (h->plan.lane_pair && h->plan.pair_stream && !h->plan.fk && !h->plan.td && kind != CDPR_COMMAND_FORCE) {
      const int new_mode = (kind == CDPR_COMMAND_VELOCITY) ? kModeVelocity : kModePosition;
      const int nbuf = h->args.pid[kind == CDPR_COMMAND_VELOCITY ? kPidVelocity : kPidPosition].nbuf;
      const int calls = (h->mode == new_mode) ? h->pid_calls : 0;  // (entering the mode resets the Pid)
      const int fill = (calls >= nbuf ? 0 : nbuf - calls) + (steps_since_load(h) == 0 ? 1 : 0);
      const int pre = ((fill + refresh_steps - 1) / refresh_steps) * refresh_steps;  // whole batches
      if (pre > 0 && pre < rest) rest = pre;
    }
    if (int rc = run_steps(h, rest, rest, record_at(done), &sched)) return rc;
    done += rest;
    j += (rest + refresh_steps - 1) / refresh_steps;
    if (j >= nbatches) c.ext[0] = d_commands + (size_t)(nbatches - 1) * batch_floats;  // the batch that stays latched
  }
  unstage.ok = true;
  return CDPR_OK;
}

}  // namespace cdpr_host
