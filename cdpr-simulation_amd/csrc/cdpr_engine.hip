// cdpr_engine.hip — host side of libcdpr_hip.so: the C-ABI of include/cdpr.h over the
// gfx950 step kernels.  No CPU compute path exists here: every entry point that
// touches robot state needs a GPU and fails with CDPR_ERR_DEVICE without one.
//
// Reference paths (relative to src/cdpr_gazebo/ of balazs-bamer/cdpr-simulation):
//   PLG.cpp = src/CdprGazeboPlugin.cpp, JFC.cpp = src/JointForceCalculator.cpp, Pid.cpp = src/Pid.cpp
#include "cdpr_engine_internal.hpp"

namespace {
thread_local std::string g_create_error;
}  // namespace

namespace cdpr_host {

// (mat3_inverse_sym, validate_config, fast_path_obstacle: cdpr_select.hpp; derivative_weights, biquad_coefficients, the Pids and every
// kernel argument: cdpr_launch_args.hpp - pure functions, shared with cdpr_plan_kernel, cdpr_debug_launch_args and the stand-alone checks)

// Cable geometry as the kernel wants it in LDS: per cable pair
// [ax0 ax1 ay0 ay1 | az0 az1 bx0 bx1 | by0 by1 bz0 bz1 | l00 l01 mask0 mask1].
std::vector<float> geom_pairs(const cdpr_config_t& c) {
  const int np = cable_pairs((int)c.n_cables);
  std::vector<float> g((size_t)np * kGeomFloatsPerPair, 0.f);
  for (int k = 0; k < np; ++k) {
    for (int h = 0; h < 2; ++h) {
      const uint32_t i = 2 * k + h;
      const bool real = i < c.n_cables;
      // the padding cable of an odd count sits far away (finite length) and is masked to zero
      const double a[3] = {real ? c.frame_anchor[i][0] : 7.0, real ? c.frame_anchor[i][1] : 11.0, real ? c.frame_anchor[i][2] : 13.0};
      const double b[3] = {real ? c.platform_anchor[i][0] : 0.0, real ? c.platform_anchor[i][1] : 0.0, real ? c.platform_anchor[i][2] : 0.0};
      float* p = &g[(size_t)k * kGeomFloatsPerPair];
      p[0 + h] = (float)a[0];
      p[2 + h] = (float)a[1];
      p[4 + h] = (float)a[2];
      p[6 + h] = (float)b[0];
      p[8 + h] = (float)b[1];
      p[10 + h] = (float)b[2];
      p[12 + h] = real ? (float)c.cable_ref_length[i] : 0.f;
      p[14 + h] = real ? 1.f : 0.f;
    }
  }
  return g;
}

int set_device(cdpr_engine* h) {
  HIP_TRY(h, hipSetDevice(h->device));
  return CDPR_OK;
}

// Host image of the state a fresh Load leaves, `rows` columns of it: platform at home, zero twist, FK seed at
// home, every controller record zero (count 0 => the first Pid call returns 0).
std::vector<float4> home_state(const cdpr_engine* h, uint32_t rows) {
  std::vector<float4> s((size_t)h->n_state * rows, make_float4(0.f, 0.f, 0.f, 0.f));
  const double* hp = h->cfg.home_pose;
  for (uint32_t r = 0; r < rows; ++r) {
    s[0 * (size_t)rows + r] = make_float4((float)hp[0], (float)hp[1], (float)hp[2], (float)hp[3]);
    s[1 * (size_t)rows + r] = make_float4((float)hp[4], (float)hp[5], (float)hp[6], 0.f);
    s[3 * (size_t)rows + r] = make_float4(0.f, (float)hp[0], (float)hp[1], (float)hp[2]);
    if (h->plan.fk) s[4 * (size_t)rows + r] = make_float4((float)hp[3], (float)hp[4], (float)hp[5], (float)hp[6]);
  }
  return s;
}

int upload_home(cdpr_engine* h) {
  HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)h->d_episode.p, (int)(uint32_t)h->origin, h->stride, h->stream));  // every episode starts at the origin (low word): age 0
  if (h->plan.fp64) return upload_home64(h);
  std::vector<float4> s = home_state(h, h->stride);
  HIP_TRY(h, hipMemcpyAsync(h->d_state, s.data(), s.size() * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  // observables before the first publish: the home pose, zeros elsewhere
  std::vector<float4> o((size_t)h->n_obs * h->stride, make_float4(0.f, 0.f, 0.f, 0.f));
  for (uint32_t r = 0; r < h->stride; ++r) {
    o[0 * (size_t)h->stride + r] = s[0 * (size_t)h->stride + r];
    o[1 * (size_t)h->stride + r] = s[1 * (size_t)h->stride + r];
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_obs, o.data(), o.size() * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  if (h->d_dbg) HIP_TRY(h, hipMemsetAsync(h->d_dbg, 0, (size_t)h->batch * CDPR_PID_DEBUG_AXES * sizeof(float), h->stream));
  for (int i = 0; i < 2; ++i)  // latched and pending Joy buffers: target 0 after Load / reset
    for (CmdChannel& c : h->cmd) HIP_TRY(h, hipMemsetAsync(c.d[i], 0, (size_t)h->stride * h->n * sizeof(float), h->stream));
  if (h->d_rec) HIP_TRY(h, hipMemsetAsync(h->d_rec, 0, h->args.glay.bytes(h->stride), h->stream));
  if (h->d_mode) HIP_TRY(h, hipMemsetAsync(h->d_mode, kModePosition, h->batch, h->stream));  // PLG.cpp:153-157 (call count 0)
  if (h->d_target) HIP_TRY(h, hipMemsetAsync(h->d_target, 0, (size_t)h->stride * h->n * sizeof(float), h->stream));  // target 0 after Load
  HIP_TRY(h, wait_stream(h));
  return CDPR_OK;
}

// Only what has an order is spelled out: both streams have drained (cdpr_destroy waits for the compute stream first), the graph
// cache goes, then the events before their streams; every buffer is an owner member and goes with the handle.
void free_all(cdpr_engine* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  h->graphs.clear();
  for (CmdChannel& c : h->cmd) {
    c.stage.clear();
    if (c.free_ev) (void)hipEventDestroy(c.free_ev);
  }
  h->reset_stage.clear(), h->copy_stage.clear();
  for (hipEvent_t ev : {h->ev0, h->ev1})
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : {h->copy_stream, h->stream})
    if (st) (void)hipStreamDestroy(st);
  delete h;
}

void engine_reset_host(cdpr_engine* h) {
  for (CmdChannel& c : h->cmd) {
    c.pending = c.masked = c.have = false;
    c.ext[0] = c.ext[1] = nullptr;
    c.sched_rows = nullptr, c.sched_mask = nullptr;
  }
  if (h->h_fault) *h->h_fault = 0u;
  h->mode = kModePosition;  // PLG.cpp:153-157: Position mode, target 0 after operator= -> reset()
  h->step = h->origin;
  h->pid_calls = 0;
  h->prev_publish = sim_time(h->origin, h->cfg.dt);  // PLG.cpp:59 (0 at origin 0)
}

// Everything the copy stream still has in flight lands before the compute stream (or the host) touches a pending buffer
// in any other way than latching it (device-side staging, masked merges, resets).
int drain_copy_stream(cdpr_engine* h) {
  if (h->copy_stream) HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
  for (CmdChannel& c : h->cmd) c.ready_wait = nullptr;
  return CDPR_OK;
}

// The rows of a command of `kind` into that kind's pending device buffer (every setter but the masked and the bound forms).
int stage_command(cdpr_engine* h, int kind, const float* src, size_t count, bool from_device) {
  const size_t n = h->n, B = h->batch;
  CmdChannel& c = h->cmd[kind];
  float* const dst = c.d[1];
  if (!src) {
    h->err = "null command buffer";
    return CDPR_ERR_INVALID;
  }
  if (count != n * B && count != n) return CDPR_IGNORED;  // PLG.cpp:68-73,77-82: silently dropped
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  const size_t bytes = n * B * sizeof(float);
  if (from_device) {
    if (int rc = drain_copy_stream(h)) return rc;
    if (count == n * B) {
      HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    } else {
      std::vector<float> one(n), all(n * B);
      HIP_TRY(h, hipMemcpy(one.data(), src, n * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t b = 0; b < B; ++b) memcpy(&all[b * n], one.data(), n * sizeof(float));
      HIP_TRY(h, hipMemcpyAsync(dst, all.data(), bytes, hipMemcpyHostToDevice, h->stream));
      HIP_TRY(h, wait_stream(h));
    }
    return CDPR_OK;
  }
  // host source: rows -> pinned staging -> pending device buffer on the copy stream, no wait for the launches in flight
  if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  if (!c.free_ev) HIP_TRY(h, hipEventCreateWithFlags(&c.free_ev, hipEventDisableTiming));
  const auto fill = [&](char* stage) {  // the whole batch, or one row for every robot
    if (count == n * B) memcpy(stage, src, bytes);
    else
      for (size_t b = 0; b < B; ++b) memcpy(stage + b * n * sizeof(float), src, n * sizeof(float));
  };
  HIP_TRY(h, c.stage.send(dst, bytes, h->copy_stream, fill, c.free_ev_set ? c.free_ev : nullptr));  // (behind every launch that read this buffer)
  c.ready_wait = c.stage.sent();
  return CDPR_OK;
}

// cdpr_create's part of a general-path handle: the controller records, sized by the layout launch_args made, and its two tables.
static int build_general(cdpr_engine* h) {
  const size_t rec_bytes = h->args.glay.bytes(h->stride);
  if (rec_bytes >= (1ull << 32)) {  // the record buffer is addressed with 32-bit offsets (one buffer resource)
    h->err = "general controller path: the controller records of this batch pass 4 GiB; split the batch over several handles";
    return CDPR_ERR_UNSUPPORTED;
  }
  CREATE_TRY(h, "hipMalloc(rec)", h->d_rec.alloc(rec_bytes));
  if (int rc = upload_table(h, h->d_gptab, h->args.ptab.data(), h->args.ptab.size() * sizeof(float), "gptab")) return rc;
  return upload_table(h, h->d_gwtab, h->args.gwtab.data(), h->args.gwtab.size() * sizeof(float), "gwtab");
}

// The handle's device pointers, batch and stride into every argument record, once, after the allocations (the list of what a launch
// still assigns: cdpr_launch_args.hpp).
static void bind_args(cdpr_engine* h) {
  for (int rec = 0; rec < kArgsRecords; ++rec) {
    const bool pr = rec == kArgsPerRobot, vel = pr || rec == kModeVelocity;
    StepArgs& a = h->args.step[rec];
    a.state = h->d_state, a.obs = h->d_obs, a.dbg = h->d_dbg, a.geom = h->d_geom;
    a.batch = h->batch, a.stride = h->stride;
    if (h->d_wtab) a.wtab = h->d_wtab + (vel ? 0 : kWin * (kWin + 2));
    if (pr && !h->plan.general) a.cmd = h->d_target, a.meta = h->d_mode;  // the robots' ACTIVE target rows, their mode / call-count bytes
    GenCtl& g = h->args.gen[rec];
    g.rec = h->d_rec, g.rstride = h->stride, g.rec_bytes = (uint32_t)h->args.glay.bytes(h->stride);
    g.mode_arr = pr ? h->d_mode.p : nullptr;
    g.wtab = h->d_gwtab, g.ptab = h->d_gptab;
    F64Args& f = h->args.f64[rec];
    f.state = h->d_state64, f.obs = h->d_obs64, f.dbg = h->d_dbg64, f.geom = h->d_geom64;
    f.batch = h->batch, f.stride = h->stride;
    if (h->d_wtab64) f.wtab = h->d_wtab64 + (vel ? 0 : win64(h->plan) * (win64(h->plan) + 2));
    if (pr) f.cmd = h->d_target, f.meta = h->d_mode;
  }
}

// Wait for the handle's stream with the host in the loop in mind (update -> synchronize -> read observables, every
// step): poll hipStreamQuery for the first kSpinUs microseconds (the blocking wait's wake-up costs 15-25 us, which is two
// step kernels; measured by scripts/short_run_probe.py), then hand over to the blocking hipStreamSynchronize so that long
// waits do not burn a core.  CDPR_SYNC_SPIN_US overrides (0 = always block).
hipError_t wait_stream(cdpr_engine* h) {
  static const long spin_us = [] {
    const char* v = std::getenv("CDPR_SYNC_SPIN_US");
    return v ? std::atol(v) : 2000L;
  }();
  if (spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) return hipSuccess;
      if (q != hipErrorNotReady) return q;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= spin_us) break;
    }
  }
  return hipStreamSynchronize(h->stream);
}

// A schedule mailbox that never delivered (cdpr_update_scheduled with d_ready): the waiting kernel gave up after its poll
// budget, raised the handle's status word and went on with whatever the schedule held - the trajectory is not what the
// caller asked for, and every call that hands results out says so until cdpr_reset.
int check_fault(cdpr_engine* h) {
  if (h->h_fault && *(volatile uint32_t*)h->h_fault != 0u) {
    h->err = "a command schedule's mailbox timed out (d_ready never became non-zero): the steps since are not the scheduled trajectory; cdpr_reset clears this";
    return CDPR_ERR_DEVICE;
  }
  return CDPR_OK;
}

// every path that hands results out ends here (include/cdpr.h: after a mailbox timeout cdpr_synchronize, the getters and
// cdpr_device_download return CDPR_ERR_DEVICE until cdpr_reset - the fp64 read-outs and the FK / TD / limit / debug getters too)
int checked(cdpr_engine* h, int rc) { return rc != CDPR_OK ? rc : check_fault(h); }

// What every kind of handle gets in cdpr_create: sizes, the argument records (launch_args), stream and events, the command buffers, the
// fp32 tables, the per-robot rows and the path's own set-up (build_f64, build_general); then the device pointers go into the records
// (bind_args), the home state is uploaded and the warm launch runs.
static int build_handle(cdpr_engine* h) {
  const cdpr_config_t& cfg = h->cfg;
  if (int rc = refuse_missing(h, missing_entry(h->plan))) return rc;  // (before anything is allocated: every kernel this plan can name has an instantiation)
  h->n = cfg.n_cables;
  h->batch = (uint32_t)cfg.batch;
  h->stride = (h->batch + 63u) & ~63u;
  // A robot's rows lie `stride` x 16 B apart.  When that is a multiple of 2 MiB (131 072 robots) every row of a wavefront
  // maps to the same HBM channels and the launch loses 17 % (131 072 x 8: 29.8 -> 24.7 us per step, 262 144: 46-54 -> 43.3;
  // profiles/r04_stride_padding.txt: this was most of "the 131 072 anomaly").  Any pad of 64 .. 1 088 columns cures it
  // alike; smaller batches are not padded (16 384: a pad costs 3-4 %).  CDPR_STRIDE_PAD=<columns> forces a pad (A/B).
  if (h->stride % 131072u == 0u) h->stride += 128u;
  // CDPR_STEP_ORIGIN=<world step>: the handle's clock starts there, and returns there on cdpr_reset (tests: the late clock in seconds).
  if (const char* so = std::getenv("CDPR_STEP_ORIGIN")) h->origin = (uint64_t)strtoull(so, nullptr, 10);
  if (const char* sp = std::getenv("CDPR_STRIDE_PAD")) h->stride = ((h->batch + 63u) & ~63u) + ((uint32_t)(std::max(0L, std::atol(sp)) + 63L) & ~63u);
  h->dbg = (cfg.stages & CDPR_STAGE_PID_DEBUG) != 0;
  if (h->plan.persist) {
    h->persist_grid = (uint32_t)h->cus * 4u;
    if (const char* pg = std::getenv("CDPR_PERSIST_GRID")) h->persist_grid = (uint32_t)std::max(1L, std::atol(pg));
  }
  h->n_state = h->plan.general ? plat_slots(h->plan.fk) : state_slots((int)h->n, h->plan.fk);
  h->n_obs = obs_slots((int)h->n);
  h->args = launch_args(cfg, h->plan);
  engine_reset_host(h);
  {
    if (const char* ss = std::getenv("CDPR_SPLIT_STEADY")) h->split_steady = !(ss[0] == '0');
    const char* ng = std::getenv("CDPR_NO_GRAPH");
    h->use_graphs = !(ng && ng[0] == '1');
  }

  CREATE_TRY(h, "hipSetDevice", hipSetDevice(h->device));
  CREATE_TRY(h, "hipStreamCreate", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CREATE_TRY(h, "hipEventCreate", hipEventCreate(&h->ev0));
  CREATE_TRY(h, "hipEventCreate", hipEventCreate(&h->ev1));
  if (h->plan.fp64) {
    if (int rc = build_f64(h)) return rc;
  } else {
    const size_t slot_bytes = (size_t)h->stride * sizeof(float4);
    CREATE_TRY(h, "hipMalloc(state)", h->d_state.alloc(slot_bytes * h->n_state));
    CREATE_TRY(h, "hipMalloc(obs)", h->d_obs.alloc(slot_bytes * h->n_obs));
  }
  const size_t cmd_bytes = (size_t)h->stride * h->n * sizeof(float);
  for (int i = 0; i < 2; ++i)
    for (CmdChannel& c : h->cmd) {
      CREATE_TRY(h, "hipMalloc(cmd)", c.d[i].alloc(cmd_bytes));
      (void)hipMemset(c.d[i], 0, cmd_bytes);
    }
  if (!h->args.wtab.empty())
    if (int rc = upload_table(h, h->d_wtab, h->args.wtab.data(), h->args.wtab.size() * sizeof(float), "wtab")) return rc;
  {
    std::vector<float> g = geom_pairs(cfg);
    if (int rc = upload_table(h, h->d_geom, g.data(), g.size() * sizeof(float), "geom")) return rc;
  }
  if (h->plan.general)
    if (int rc = build_general(h)) return rc;
  if (h->plan.per_robot) {
    if (!h->plan.general) CREATE_TRY(h, "hipMalloc(target)", h->d_target.alloc(cmd_bytes));
    CREATE_TRY(h, "hipMalloc(mode)", h->d_mode.alloc(h->batch));
    for (CmdChannel& c : h->cmd) CREATE_TRY(h, "hipMalloc(mask)", c.d_mask.alloc(h->batch));
  }
  CREATE_TRY(h, "hipMalloc(episode)", h->d_episode.alloc((size_t)h->stride * sizeof(uint32_t)));
  if (h->dbg && !h->plan.fp64) CREATE_TRY(h, "hipMalloc(dbg)", h->d_dbg.alloc((size_t)h->batch * CDPR_PID_DEBUG_AXES * sizeof(float)));
  bind_args(h);
  if (upload_home(h) != CDPR_OK || warm_first_launch(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return CDPR_OK;
}

}  // namespace cdpr_host

// =================================================================================
// C-ABI
// =================================================================================
extern "C" {

uint32_t cdpr_abi_version(void) { return CDPR_ABI_VERSION; }
size_t cdpr_config_size(void) { return sizeof(cdpr_config_t); }

int cdpr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cdpr_device_pci_bus_id(int device, char* out, size_t len) {
  if (!out || len < 13) return CDPR_ERR_INVALID;
  out[0] = 0;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return CDPR_ERR_INVALID;
  if (hipDeviceGetPCIBusId(out, (int)len, device) != hipSuccess) return CDPR_ERR_DEVICE;
  return CDPR_OK;
}

size_t cdpr_bytes_per_state_step(const cdpr_config_t* cfg) {
  // read command n; read+write platform 13 and controller 12 per cable;
  // write observables 13 + 3n.  4 * (39 + 28 n).
  if (!cfg) return 0;
  return 4u * (39u + 28u * (size_t)cfg->n_cables);
}

int cdpr_derivative_weights(uint32_t n, uint32_t degree, double* w) {
  if (!w) return CDPR_ERR_INVALID;
  return derivative_weights(n, degree, w);
}

const char* cdpr_last_error(cdpr_handle_t h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int cdpr_create(const cdpr_config_t* cfg, int device, cdpr_handle_t* out) {
  if (out) *out = nullptr;
  if (!cfg || !out) {
    g_create_error = "null argument";
    return CDPR_ERR_INVALID;
  }
  // the routing of this configuration (which kernel family, which mapping): cdpr_select.hpp, a pure function of the
  // configuration shared with cdpr_plan_kernel; 256 CUs assumed until the device is known (re-planned below)
  KernelPlan plan = plan_kernels(*cfg);
  if (plan.rc != CDPR_OK) {
    g_create_error = plan.error;
    return plan.rc;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible (this engine has no CPU path)";
    return CDPR_ERR_DEVICE;
  }
  if (device < 0 || device >= ndev) {
    g_create_error = "device index out of range";
    return CDPR_ERR_INVALID;
  }
  cdpr_engine* h = new cdpr_engine();
  h->cfg = *cfg;
  h->device = device;
  if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->cus <= 0) h->cus = 256;
  h->plan = plan_kernels(*cfg, h->cus);  // (the general path's role-split limit follows the device's CU count)
  // every failure from here on releases what the handle has got so far and leaves *out null
  const int rc = build_handle(h);
  if (rc != CDPR_OK) {
    g_create_error = h->err;
    free_all(h);
    return rc;
  }
  *out = h;
  return CDPR_OK;
}

void cdpr_destroy(cdpr_handle_t h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_all(h);
}

int cdpr_reset(cdpr_handle_t h) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (int rc = drain_copy_stream(h)) return rc;
  HIP_TRY(h, wait_stream(h));
  for (CmdChannel& c : h->cmd) c.free_ev_set = false;
  engine_reset_host(h);
  return upload_home(h);
}

// A pending command replaces the one before it (PLG.cpp:69,78: the callback overwrites the stored message); on a
// per-robot handle an UNMASKED command after a masked one would have to merge with it, which the callbacks of
// independent plugins never need: the later call wins for the robots it addresses, the earlier one keeps the rest.
static int stage_masked(cdpr_engine* h, int kind, const float* axes, size_t count, const uint8_t* robot_mask) {
  if (!h) return CDPR_ERR_INVALID;
  if (!axes) {
    h->err = "null command buffer";
    return CDPR_ERR_INVALID;
  }
  if (!h->plan.per_robot) {
    h->err = "masked commands need a handle created with per_robot_commands = 1";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (!robot_mask) {
    h->err = "null robot mask";
    return CDPR_ERR_INVALID;
  }
  const size_t n = h->n, B = h->batch;
  if (count != n * B && count != n) return CDPR_IGNORED;  // PLG.cpp:68-73,77-82
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (int rc = drain_copy_stream(h)) return rc;
  CmdChannel& c = h->cmd[kind];
  // merge with a command of the same kind that is already pending: rows and mask bits of the robots addressed now
  std::vector<float> rows(n * B);
  std::vector<uint8_t> mask(B, 0);
  if (c.pending) {
    HIP_TRY(h, hipMemcpyAsync(rows.data(), c.d[1], n * B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (c.masked)
      HIP_TRY(h, hipMemcpyAsync(mask.data(), c.d_mask, B, hipMemcpyDeviceToHost, h->stream));
    else
      std::fill(mask.begin(), mask.end(), (uint8_t)1);
    HIP_TRY(h, wait_stream(h));
  }
  for (size_t b = 0; b < B; ++b) {
    if (!robot_mask[b]) continue;
    mask[b] = 1;
    memcpy(&rows[b * n], count == n ? axes : axes + b * n, n * sizeof(float));
  }
  HIP_TRY(h, hipMemcpyAsync(c.d[1], rows.data(), n * B * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c.d_mask, mask.data(), B, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, wait_stream(h));
  c.pending = true;
  c.masked = true;
  return CDPR_OK;
}

// The unmasked setters, host or device source: the rows replace whatever of that kind was pending, a bound buffer included.
static int set_command(cdpr_engine* h, int kind, const float* axes, size_t count, bool from_device) {
  if (!h) return CDPR_ERR_INVALID;
  const int rc = stage_command(h, kind, axes, count, from_device);
  if (rc == CDPR_OK) {
    CmdChannel& c = h->cmd[kind];
    c.pending = true;
    c.masked = false;
    c.ext[1] = nullptr;
  }
  return rc;
}

// Zero-copy form: the caller's device buffer float[B][n] IS the latched Joy batch from the next update on (no copy, no
// synchronisation); it must stay valid and unchanged until another command of the same kind has been latched.
static int bind_command(cdpr_engine* h, int kind, const float* d_axes, size_t count) {
  if (!h) return CDPR_ERR_INVALID;
  if (!d_axes) {
    h->err = "null command buffer";
    return CDPR_ERR_INVALID;
  }
  if (count != (size_t)h->n * h->batch) return CDPR_IGNORED;  // one Joy per robot; no broadcast without a copy
  if (h->plan.per_robot) {
    h->err = "cdpr_bind_*_command_device: not available on a per_robot_commands handle (commands are latched robot by robot)";
    return CDPR_ERR_UNSUPPORTED;
  }
  h->cmd[kind].ext[1] = d_axes;
  h->cmd[kind].pending = true;
  return CDPR_OK;
}

int cdpr_set_velocity_command(cdpr_handle_t h, const float* axes, size_t count) { return set_command(h, CDPR_COMMAND_VELOCITY, axes, count, false); }
int cdpr_set_position_command(cdpr_handle_t h, const float* axes, size_t count) { return set_command(h, CDPR_COMMAND_POSITION, axes, count, false); }
int cdpr_set_force_command(cdpr_handle_t h, const float* axes, size_t count) { return set_command(h, CDPR_COMMAND_FORCE, axes, count, false); }

int cdpr_set_velocity_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return set_command(h, CDPR_COMMAND_VELOCITY, d_axes, count, true); }
int cdpr_set_position_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return set_command(h, CDPR_COMMAND_POSITION, d_axes, count, true); }
int cdpr_set_force_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return set_command(h, CDPR_COMMAND_FORCE, d_axes, count, true); }

int cdpr_set_velocity_command_masked(cdpr_handle_t h, const float* axes, size_t count, const uint8_t* robot_mask) {
  return stage_masked(h, CDPR_COMMAND_VELOCITY, axes, count, robot_mask);
}
int cdpr_set_position_command_masked(cdpr_handle_t h, const float* axes, size_t count, const uint8_t* robot_mask) {
  return stage_masked(h, CDPR_COMMAND_POSITION, axes, count, robot_mask);
}
int cdpr_set_force_command_masked(cdpr_handle_t h, const float* axes, size_t count, const uint8_t* robot_mask) {
  return stage_masked(h, CDPR_COMMAND_FORCE, axes, count, robot_mask);
}

int cdpr_bind_velocity_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return bind_command(h, CDPR_COMMAND_VELOCITY, d_axes, count); }
int cdpr_bind_position_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return bind_command(h, CDPR_COMMAND_POSITION, d_axes, count); }
int cdpr_bind_force_command_device(cdpr_handle_t h, const float* d_axes, size_t count) { return bind_command(h, CDPR_COMMAND_FORCE, d_axes, count); }

int cdpr_update(cdpr_handle_t h, int nsteps) { return run_steps(h, nsteps, 1); }

int cdpr_update_fused(cdpr_handle_t h, int nsteps, int steps_per_launch) { return run_steps(h, nsteps, steps_per_launch); }

int cdpr_observable_image_bytes(cdpr_handle_t h, size_t* bytes) {
  if (!h || !bytes) return CDPR_ERR_INVALID;
  *bytes = image_bytes(h);
  return CDPR_OK;
}

int cdpr_update_record(cdpr_handle_t h, int nsteps, int steps_per_launch, void* d_record, size_t record_bytes) {
  if (!h) return CDPR_ERR_INVALID;
  if (h->cfg.publish_period != 0.0) {
    h->err = "cdpr_update_record needs publish_period == 0 (every step published)";
    return CDPR_ERR_UNSUPPORTED;
  }
  const size_t image = image_bytes(h);
  if (!d_record || nsteps < 0 || record_bytes < image * (size_t)nsteps) {
    h->err = "cdpr_update_record: record buffer missing or smaller than nsteps observable images";
    return CDPR_ERR_INVALID;
  }
  return run_steps(h, nsteps, steps_per_launch, d_record);
}

int cdpr_update_scheduled(cdpr_handle_t h, int nsteps, int refresh_steps, const float* d_commands, const uint32_t* d_ready, void* d_record,
                          size_t record_bytes) {
  if (!h) return CDPR_ERR_INVALID;
  return scheduled_update(h, CDPR_COMMAND_VELOCITY, nsteps, refresh_steps, d_commands, d_ready, nullptr, d_record, record_bytes);
}

int cdpr_update_scheduled_kind(cdpr_handle_t h, uint32_t kind, int nsteps, int refresh_steps, const float* d_commands, const uint32_t* d_ready,
                               const uint8_t* d_robot_masks, void* d_record, size_t record_bytes) {
  if (!h) return CDPR_ERR_INVALID;
  return scheduled_update(h, kind, nsteps, refresh_steps, d_commands, d_ready, d_robot_masks, d_record, record_bytes);
}

int cdpr_synchronize(cdpr_handle_t h) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, wait_stream(h));
  return checked(h, CDPR_OK);
}

static int copy_name(const std::string& text, char* name, size_t len) {
  if (!name || len == 0) return CDPR_ERR_INVALID;
  const size_t k = std::min(text.size(), len - 1);
  memcpy(name, text.data(), k);
  name[k] = 0;
  return CDPR_OK;
}

static LaunchShape shape_of_flags(int steps_per_launch, uint32_t flags) {
  LaunchShape s;
  s.steps = steps_per_launch;
  s.first_world = (flags & CDPR_PLAN_FIRST_WORLD_STEP) != 0u;
  s.scheduled = (flags & CDPR_PLAN_SCHEDULED) != 0u;
  s.rollout = (flags & CDPR_PLAN_ROLLOUT) != 0u;
  s.steady = (flags & CDPR_PLAN_NOT_STEADY) == 0u;
  return s;
}

int cdpr_plan_kernel(const cdpr_config_t* cfg, int steps_per_launch, uint32_t flags, char* name, size_t len) {
  if (!cfg || !name || len == 0 || steps_per_launch < 1) return CDPR_ERR_INVALID;
  const KernelPlan plan = plan_kernels(*cfg);  // (no HIP call: works on a box without a GPU)
  if (plan.rc != CDPR_OK) {
    copy_name(plan.error, name, len);
    return plan.rc;
  }
  return copy_name(planned_kernel_name(planned_kernel(plan, shape_of_flags(steps_per_launch, flags))), name, len);
}

// Is there an instantiation behind the kernel cdpr_plan_kernel names for these arguments?  1: yes - in both modes and, where the kernel
// has one, in its steady-state form too (missing_entry, cdpr_kernels.hpp); 0: a lookup came back empty; the refusal's code where the
// configuration is refused.  From the configuration alone, no HIP call.  For tests, not part of the C-ABI header.
int cdpr_debug_plan_entry(const cdpr_config_t* cfg, int steps_per_launch, uint32_t flags) {
  if (!cfg || steps_per_launch < 1) return CDPR_ERR_INVALID;
  const KernelPlan plan = plan_kernels(*cfg);
  if (plan.rc != CDPR_OK) return plan.rc;
  return missing_entry(plan, shape_of_flags(steps_per_launch, flags)).id == KernelId::None ? 1 : 0;
}
// The bytes of the argument records a launch of a handle of this configuration copies in `mode` (0 Force, 1 Position, 2 Velocity), pointers
// null and the per-launch fields zero, the path's uploaded tables appended (launch_args_image, cdpr_launch_args.hpp): written to buf where
// len suffices; returns their count, or the refusal's code.  From the configuration alone, no HIP call.  For tests, not part of the C-ABI header.
int cdpr_debug_launch_args(const cdpr_config_t* cfg, int mode, void* buf, size_t len) {
  if (!cfg || mode < kModeForce || mode > kModeVelocity) return CDPR_ERR_INVALID;
  const KernelPlan plan = plan_kernels(*cfg);
  if (plan.rc != CDPR_OK) return plan.rc;
  const std::vector<unsigned char> image = launch_args_image(launch_args(*cfg, plan), plan, mode);
  if (buf && len >= image.size()) memcpy(buf, image.data(), image.size());
  return (int)image.size();
}
// ... and the entry point itself (of the form cdpr_plan_kernel names: Position mode, not the steady-state instantiation), null where
// there is none or the configuration is refused: two cells run the same code exactly where these are equal
const void* cdpr_debug_plan_entry_address(const cdpr_config_t* cfg, int steps_per_launch, uint32_t flags) {
  if (!cfg || steps_per_launch < 1) return nullptr;
  const KernelPlan plan = plan_kernels(*cfg);
  return plan.rc != CDPR_OK ? nullptr : entry_address(planned_kernel(plan, shape_of_flags(steps_per_launch, flags)));
}

int cdpr_kernel_name(cdpr_handle_t h, char* name, size_t len) {
  if (!h) return CDPR_ERR_INVALID;
  return copy_name(planned_kernel_name(h->last_kernel), name, len);
}

uint32_t cdpr_mapping(cdpr_handle_t h) {
  return !h ? CDPR_MAP_AUTO : (h->plan.lane_cable ? CDPR_MAP_LANE_PER_CABLE : h->plan.lane_pair ? CDPR_MAP_LANE_PAIR : CDPR_MAP_LANE_PER_ROBOT);
}

uint64_t cdpr_step_count(cdpr_handle_t h) { return h ? h->step : 0; }

// Which instantiation the last step launch of run_steps took: 0 = the planned kernel as cdpr_kernel_name gives it, 1 = the role-split
// kernel's steady-state instantiation (PlannedKernel::steady of h->last_kernel).  Host-side state; for tests and A/B scripts, not part of the C-ABI header.
int cdpr_debug_last_variant(cdpr_handle_t h) { return h ? (h->last_kernel.steady ? 1 : 0) : -1; }

#ifdef CDPR_STAMPS
// diagnostic builds only: point the step kernel at a stamp buffer (uint64[blocks][8]); nullptr disables
int cdpr_debug_set_stamps(cdpr_handle_t h, unsigned long long* d_stamps) {
  if (!h) return CDPR_ERR_INVALID;
  for (int rec = 0; rec < kArgsRecords; ++rec) h->args.step[rec].stamps = h->args.f64[rec].stamps = d_stamps;  // every record a later launch copies
  return CDPR_OK;
}
#endif

int cdpr_device_malloc(cdpr_handle_t h, size_t bytes, void** out) {
  if (!h || !out) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipMalloc(out, bytes));
  return CDPR_OK;
}

int cdpr_device_free(cdpr_handle_t h, void* ptr) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipFree(ptr));
  return CDPR_OK;
}

int cdpr_device_upload(cdpr_handle_t h, void* dst, const void* src, size_t bytes) {
  if (!h || !dst || !src) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, wait_stream(h));
  return CDPR_OK;
}

int cdpr_device_download(cdpr_handle_t h, void* dst, const void* src, size_t bytes) {
  if (!h || !dst || !src) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, wait_stream(h));
  return checked(h, CDPR_OK);  // (a trajectory record of a schedule whose mailbox timed out is not the scheduled one)
}

int cdpr_profile_begin(cdpr_handle_t h) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  h->launches_mark = h->launches;
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  return CDPR_OK;
}

int cdpr_profile_end(cdpr_handle_t h, float* elapsed_ms, uint64_t* kernel_launches) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  // ONE wait for everything queued on the stream, the closing event included.  (hipEventSynchronize followed by the
  // caller's hipStreamSynchronize costs two wake-ups: measured 28 us on a 20-launch timed region, scripts/short_run_probe.py.)
  HIP_TRY(h, wait_stream(h));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (elapsed_ms) *elapsed_ms = ms;
  if (kernel_launches) *kernel_launches = h->launches - h->launches_mark;
  return CDPR_OK;
}

}  // extern "C"
