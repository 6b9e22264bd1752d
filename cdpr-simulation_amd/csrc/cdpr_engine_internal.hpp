// cdpr_engine_internal.hpp - what the translation units of the host side share: the owners of device and pinned memory and of the
// captured graphs (DevBuf, PinnedBuf, StagePair, GraphCache), the views of a per-robot handle's records with the one launch helper
// of the kernels over chosen robots (fast_records / gen_records / f64_records, launch_per_robot), the handle (struct cdpr_engine: its routing is h->plan and nothing else, its
// buffers are owner members that go with it, its kernel arguments are h->args: cdpr_launch_args.hpp), the error macros and the helpers one unit defines and another calls.  Units:
// cdpr_engine.hip (create / destroy with bind_args, the general path's set-up, the command setters, the extern "C" wrappers), cdpr_engine_readout.hip (the getters,
// the image decoders and cdpr_set_platform_state* on the column table of cdpr_readout.hpp: one gather kernel, read_blocks),
// cdpr_engine_launch.hip (what turns "advance n world steps" into launches: the latch, the chain and its clock, the fp32 and
// general paths, schedules), cdpr_engine_f64.hip (precision = 64: set-up, its path of the chain), cdpr_engine_rollout.hip (cdpr_rollout_velocity*), cdpr_engine_solvers.hip (cdpr_solve_ik / fk / td), cdpr_engine_reset.hip
// (cdpr_reset_robots*), cdpr_engine_copy.hip (cdpr_copy_robots*), cdpr_engine_done.hip (cdpr_evaluate_done*, cdpr_reset_done_device, cdpr_get_episode_start), cdpr_engine_env.hip (cdpr_observe_device,
// cdpr_env_evaluate_device, cdpr_observation_width), cdpr_engine_resample.hip (cdpr_resample_map_device, cdpr_resample_device),
// cdpr_engine_mppi.hip (cdpr_mppi_sample_device, cdpr_mppi_update_device), cdpr_engine_cem.hip (cdpr_cem_sample_device,
// cdpr_cem_update_device).  Not installed, not part of the C-ABI (include/cdpr.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/cdpr.h"
#include "cdpr_launch_args.hpp"
#include "cdpr_robot_records.hpp"
#include "cdpr_solvers.hpp"
#include "cdpr_readout.hpp"

using namespace cdpr;

namespace cdpr_host {

#define HIP_TRY(h, expr)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                              \
      return CDPR_ERR_DEVICE;                                                                    \
    }                                                                                            \
  } while (0)

// a failed step of cdpr_create: the message into the handle, the code the ABI returns (cdpr_create hands both on and frees the handle)
#define CREATE_TRY(h, what, expr)                                                                \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (h)->err = std::string(what) + ": " + hipGetErrorString(e_);                               \
      return e_ == hipErrorOutOfMemory ? CDPR_ERR_NOMEM : CDPR_ERR_DEVICE;                       \
    }                                                                                            \
  } while (0)

}  // namespace cdpr_host
struct cdpr_engine;
namespace cdpr_host {

hipError_t wait_stream(cdpr_engine* h);  // poll, then block (cdpr_engine.hip)

// The owner of one device allocation (cap bytes): freed with its owner - the handle, or a function's scratch.  Reads as the T* it holds.
template <typename T = void>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
  hipError_t alloc(size_t bytes) {
    release();
    const hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 4);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  // grow-only scratch: a buffer too short is replaced once the handle's stream, which may still use it, has drained; a failed
  // allocation leaves p null and cap 0
  hipError_t ensure(cdpr_engine* h, size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    const hipError_t e = wait_stream(h);
    return e != hipSuccess ? e : alloc(bytes);
  }
  void swap(DevBuf& o) { std::swap(p, o.p), std::swap(cap, o.cap); }
  operator T*() const { return p; }
  template <typename U> U* as() const { return static_cast<U*>(p); }
};

// ... and of one pinned host allocation (hipHostMalloc)
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t bytes, unsigned flags) { return hipHostMalloc((void**)&p, bytes, flags); }
  operator T*() const { return p; }
};

// ... and of two pinned blocks that take turns on the way to the device, each with the event of its last copy: what a host-form call
// hands over goes into the free block (the caller's arrays are its own again on return) and from there to the device on a stream.
// The call that fills a block waits only for the copy of two calls back, never for the stream.  Allocated at first use (every use of
// one StagePair sends the same number of bytes).
struct StagePair {
  PinnedBuf<char> block[2];
  hipEvent_t ev[2] = {nullptr, nullptr};  // the copy out of that block has completed
  bool ev_set[2] = {false, false};
  int idx = 0;
  StagePair() = default;
  StagePair(const StagePair&) = delete;
  StagePair& operator=(const StagePair&) = delete;
  ~StagePair() { clear(); }
  void clear() {  // (before the streams go: free_all)
    for (int i = 0; i < 2; ++i) {
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      ev[i] = nullptr, ev_set[i] = false;
    }
  }
  // fill(char*) writes `bytes` into the free block, which then travels to d_dst on `stream` - behind `after`, if one is given (queued
  // right in front of the copy, so that the two reach the stream together)
  template <typename Fill>
  hipError_t send(void* d_dst, size_t bytes, hipStream_t stream, Fill&& fill, hipEvent_t after = nullptr) {
    idx ^= 1;
    hipError_t e = block[idx] ? hipSuccess : block[idx].alloc(bytes, hipHostMallocDefault);
    if (e == hipSuccess && !ev[idx]) e = hipEventCreateWithFlags(&ev[idx], hipEventDisableTiming);
    if (e == hipSuccess && ev_set[idx]) e = hipEventSynchronize(ev[idx]);  // two calls back: long done
    if (e != hipSuccess) return e;
    fill(block[idx].p);
    if (after && (e = hipStreamWaitEvent(stream, after, 0)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_dst, block[idx], bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipEventRecord(ev[idx], stream)) == hipSuccess) ev_set[idx] = true;
    return e;
  }
  hipEvent_t sent() const { return ev[idx]; }  // the copy of the last send() has completed
};

// ... and of the captured hipGraphs of a handle: chains of identical steady-state launches (run_steps), found again by what makes
// two chains the same launches - kernel, command pointer, steps per launch, flags and the ring slot the chain starts from.
struct GraphKey {
  void* kern; const float* cmd; int steps_per_launch, start_slot; uint32_t flags;
  bool operator==(const GraphKey& o) const { return kern == o.kern && cmd == o.cmd && steps_per_launch == o.steps_per_launch && start_slot == o.start_slot && flags == o.flags; }
};
struct GraphCache {
  struct Entry { GraphKey key; hipGraph_t graph; hipGraphExec_t exec; };
  std::vector<Entry> entries;  // oldest first; 32 at the most (two Joy buffers x a few ring positions x step counts)
  GraphCache() = default;
  GraphCache(const GraphCache&) = delete;
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() { clear(); }
  void evict(size_t count) {  // the `count` oldest
    for (size_t i = 0; i < count; ++i) (void)hipGraphExecDestroy(entries[i].exec), (void)hipGraphDestroy(entries[i].graph);
    entries.erase(entries.begin(), entries.begin() + count);
  }
  void clear() { evict(entries.size()); }
  hipGraphExec_t find(const GraphKey& key) const {
    for (const Entry& e : entries)
      if (e.key == key) return e.exec;
    return nullptr;
  }
  // What `launch_all` queues on `stream` (it says whether every launch took) as a graph under `key`.  The capture is ended on every
  // path - the stream is never left capturing; a failure anywhere drops the partial graph and returns null: do not use graphs on
  // this handle again.
  template <typename Fn>
  hipGraphExec_t capture(hipStream_t stream, const GraphKey& key, Fn&& launch_all) {
    Entry e{key, nullptr, nullptr};
    bool ok = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const bool launched = launch_all();
      ok = (hipStreamEndCapture(stream, &e.graph) == hipSuccess) && launched && e.graph;
      if (ok && hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
      if (!ok && e.graph) (void)hipGraphDestroy(e.graph);
    }
    if (!ok) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (entries.size() >= 32) evict(1);
    entries.push_back(e);
    return e.exec;
  }
};

// Everything one command kind owns.  The handle keeps one record per kind, cdpr_engine::cmd[], indexed by the ABI's
// CDPR_COMMAND_VELOCITY / _POSITION / _FORCE (0, 1, 2); what differs between the kinds is kCmdKind below.
struct CmdChannel {
  DevBuf<float> d[2];                        // the engine's own device buffers: [0] latched, [1] pending
  // zero-copy commands (cdpr_bind_*_command_device): a caller-owned device buffer takes the place of d[0] / d[1]
  const float* ext[2] = {nullptr, nullptr};
  DevBuf<uint8_t> d_mask;                    // per-robot handles: the pending command's mask, uint8[B]
  bool pending = false;
  bool masked = false;                       // the pending command came with a mask
  bool have = false;                         // a command of this kind has been latched since Load
  // Host-side Joy batches travel on their own stream (cdpr_set_*_command with a host pointer): the caller's rows go into
  // one of two pinned staging buffers and from there to the PENDING device buffer while earlier launches still
  // run; the call returns without waiting.
  StagePair stage;
  hipEvent_t ready_wait = nullptr;  // event the compute stream has to pass before it touches the pending buffer
  hipEvent_t free_ev = nullptr;     // every launch that read what is now the pending buffer has completed
  bool free_ev_set = false;
  // cdpr_update_scheduled_kind on a per-robot handle: batch j of the schedule is latched straight from the caller's device
  // buffers (rows d_commands + j * B * n, mask d_robot_masks + j * B or nullptr = every robot), nothing staged
  const float* sched_rows = nullptr;
  const uint8_t* sched_mask = nullptr;

  const float* latched() const { return ext[0] ? ext[0] : d[0].p; }  // what the launches read: the bound buffer where one is latched
};

constexpr int kCmdKinds = 3;
struct CmdKind {
  int mode;        // the mode a latched command of this kind enters
  int reset_pid;   // the Pid a CHANGE of mode resets (general path / hold rows: 0 = position, 1 = velocity), -1: none
  uint32_t meta;   // the mode as the per-robot latch kernels take it (StepArgs::meta)
};
// in latch order: velocity, position (PLG.cpp:206-219), then force ([NEW]: the reference has no force callback)
constexpr CmdKind kCmdKind[kCmdKinds] = {
    {kModeVelocity, 1, kMetaVelocity},   // CDPR_COMMAND_VELOCITY: setVelocityTarget, JFC.cpp:113-115
    {kModePosition, 0, kMetaPosition},   // CDPR_COMMAND_POSITION: setPositionTarget, JFC.cpp:101-103
    {kModeForce, -1, kMetaForce},        // CDPR_COMMAND_FORCE: setForce, JFC.h:92-95 (no Pid is reset)
};
static_assert(CDPR_COMMAND_VELOCITY == 0 && CDPR_COMMAND_POSITION == 1 && CDPR_COMMAND_FORCE == 2, "kCmdKind is indexed by the ABI's command kinds");

}  // namespace cdpr_host
using namespace cdpr_host;

struct cdpr_engine {
  cdpr_config_t cfg{};
  KernelPlan plan;          // the routing cdpr_create took for this configuration (cdpr_select.hpp): the only copy, every reader takes h->plan.X
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t n = 0, batch = 0, stride = 0;
  bool dbg = false;
  int n_state = 0, n_obs = 0;
  DevBuf<float4> d_state, d_obs;
  DevBuf<float> d_dbg;
  DevBuf<float> d_geom;     // pair-interleaved cable geometry, staged in LDS by the kernel
  int pid_calls = 0;        // Pid::update calls since the last Pid reset (uniform over the batch)
  uint32_t persist_grid = 0;  // waves of a launch of the persistent one-wave kernel (plan.persist): SIMDs of the device
  PinnedBuf<uint32_t> h_fault;      // pinned, device-mapped status word: a schedule mailbox that never delivered (kernels OR bits into it)
  uint32_t* d_fault = nullptr;      // its device address
  // general controller path (hold branch, cascades, long windows): see cdpr_general_step.hpp
  DevBuf<float> d_rec;       // record rows: [mLastPosition per cable][position Pid rows][velocity Pid rows], one column per robot
  DevBuf<float> d_gwtab;     // FIR weights by ring head, [pid][head][slot]
  DevBuf<float> d_gptab;     // the two Pids' parameters as the kernel stages them in LDS (gen_pid_table)
  // MPC rollout on a precision = 64 handle: the trajectories' state rows, their cost accumulators, the step's Joy batch,
  // per-robot handles: every trajectory's mode / Pid call count byte.  Grow-only, sized together for roll64_cols columns (their row stride)
  DevBuf<double> d_roll64, d_roll64_acc;
  DevBuf<float> d_roll64_cmd;
  DevBuf<uint8_t> d_roll64_meta;
  size_t roll64_cols = 0;
  DevBuf<float> d_roll_rec;      // MPC rollout on the general path: every trajectory's private copy of the records
  size_t roll_rec_cols = 0;      // columns d_roll_rec can hold
  GraphCache graphs;          // chains of identical steady-state launches (run_steps)
  PlannedKernel last_kernel;  // what the last step launch ran on (cdpr_kernel_name; its `steady`: cdpr_debug_last_variant)
  bool split_steady = true;   // CDPR_SPLIT_STEADY=0: the role-split kernel always runs its generic instantiation
  int cus = 256;
  bool use_graphs = true;
  CmdChannel cmd[kCmdKinds];  // command state, one record per kind
  // per-robot command arrival (plan.per_robot): every robot has its own mode
  DevBuf<uint8_t> d_mode;           // uint8[B]: 1 = Position, 2 = Velocity; on the register-resident path also the robot's
                                    // Pid call count in bits 2-7 (StepArgs::meta)
  DevBuf<float> d_target;           // per-robot handles on the register-resident path: float[B][n], every robot's ACTIVE target row
  hipStream_t copy_stream = nullptr;  // host-side Joy batches travel on their own stream (CmdChannel::stage)
  int mode = kModePosition;
  uint64_t step = 0;
  uint64_t origin = 0;           // the world step a fresh or reset handle stands at (CDPR_STEP_ORIGIN, read once by cdpr_create; default 0)
  double prev_publish = 0.0;
  LaunchArgs args;                // every kernel argument that outlives a launch (cdpr_launch_args.hpp): made by cdpr_create, device pointers bound in (bind_args)
  DevBuf<float> d_wtab;           // register-resident path: args.wtab on the device
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint64_t launches = 0, launches_mark = 0;
  // read-out (read_blocks, cdpr_engine_readout.hip): device scratch the gather writes where it does not store to the host itself
  // (grow-only), the pinned, device-mapped host image of the small tiers, the completion word with its arrival counter and epoch
  DevBuf<char> d_unpack;
  PinnedBuf<char> h_pub;
  PinnedBuf<uint64_t> h_pub_done;
  DevBuf<uint32_t> d_pub_arrivals;
  uint64_t pub_epoch = 0;
  // MPC rollout scratch, persistent and grow-only (no hipMalloc / hipFree inside a rollout that fits)
  DevBuf<float> d_roll_ref;      // float[B][3]
  DevBuf<float> d_roll_cost;     // float[B][samples]
  uint64_t roll_pending = 0;     // trajectories of the launched, not yet fetched rollout
  // cdpr_reset_robots (host form): the caller's mask, poses and twists go through a pinned staging pair into persistent device
  // scratch on the handle's stream ([uint8 mask[B], padded to 16 B | float pose[B][7] | float twist[B][6]], sized once: B is fixed)
  DevBuf<char> d_reset_args;
  StagePair reset_stage;
  // cdpr_copy_robots (host form): the caller's source map, staged the same way (int32[B], sized once); also the map of
  // cdpr_resample_device where the caller gives none
  DevBuf<int32_t> d_copy_map;
  StagePair copy_stage;
  // episode clock: uint32[stride], the world step (low word) of every robot's last model reset; zero after create / cdpr_reset and
  // on uniform handles.  d_done: scratch of cdpr_evaluate_done's host form and the mask of cdpr_reset_done_device
  // ([uint8 mask[B], padded to 16 B | uint32 reason[B] | uint32 counts[CDPR_DONE_COUNTS]], sized once)
  DevBuf<uint32_t> d_episode;
  DevBuf<char> d_done;
  // cdpr_config_t.precision = 64 (plan.fp64): the step in double (cdpr_step_kernel_f64.hpp); its own state, observables, tables
  DevBuf<double> d_state64, d_obs64;
  DevBuf<double> d_geom64;       // [n][7]
  DevBuf<double> d_wtab64;       // [velocity | position] x [10][12]
  DevBuf<double> d_dbg64;
  std::string err;
};

namespace cdpr_host {


// a device copy of a host table (cdpr_create)
template <typename T>
int upload_table(cdpr_engine* h, DevBuf<T>& d, const void* src, size_t bytes, const char* name) {
  CREATE_TRY(h, "hipMalloc(" + std::string(name) + ")", d.alloc(bytes));
  CREATE_TRY(h, "hipMemcpy(" + std::string(name) + ")", hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
  return CDPR_OK;
}

// the kind whose latched command a uniform handle in `mode` reads
inline int cmd_kind_of_mode(int mode) { return mode == kModeVelocity ? (int)CDPR_COMMAND_VELOCITY : mode == kModeForce ? (int)CDPR_COMMAND_FORCE : (int)CDPR_COMMAND_POSITION; }

// The argument record of the handle's current mode; the controller half of a general-path launch with the latched commands (null: none yet, target 0)
inline int args_index(const cdpr_engine* h) { return args_index(h->plan, h->mode); }
inline GenCtl general_ctl(const cdpr_engine* h) {
  GenCtl g = h->args.gen[args_index(h)];
  const auto latched = [h](int kind) { return h->cmd[kind].have ? h->cmd[kind].latched() : nullptr; };
  g.vel_cmd = latched(CDPR_COMMAND_VELOCITY), g.pos_cmd = latched(CDPR_COMMAND_POSITION), g.frc_cmd = latched(CDPR_COMMAND_FORCE);
  return g;
}

constexpr int kCallSat = 64;  // Pid call counts saturate here on the host (the kernels ask "0?", ">= nbuf?")
inline int sat_pid_calls(int calls) { return calls < kCallSat ? calls : kCallSat; }
// World steps since Load (cdpr_create, cdpr_reset): the clock starts at h->origin, so "the first update has not run yet" is
// steps_since_load(h) == 0 - the only spelling of that test on the host.
inline uint64_t steps_since_load(const cdpr_engine* h) { return h->step - h->origin; }
// The general controller path keeps world-step stamps as int32 (controller records, hot rows; GenCtl::now_step): a call that would take
// the counter to 2^31 is refused - before a command is latched or a launch queued, so the handle is as it was.
inline int general_clock_check(cdpr_engine* h, uint64_t nsteps) {
  if (h->plan.general && h->step + nsteps >= (1ull << 31)) {
    h->err = "general controller path: world-step counter would pass 2^31";
    return CDPR_ERR_UNSUPPORTED;
  }
  return CDPR_OK;
}
// ring slot the error of world step `step` is written to (fp32 kernels: a ring of kWin; fp64: of w = win64)
inline int ring_slot_of(uint64_t step) { return (int)((step + 8u) % (uint64_t)kWin); }
inline int ring_slot_of(uint64_t step, int w) { return (int)((step + (uint64_t)(w - 2)) % (uint64_t)w); }

// A cdpr_update_scheduled launch in progress (run_steps' last argument; null for a plain update): Joy batches `refresh` steps apart
// read by the kernel itself (StepArgs::sched_*), their mailbox or null, the status word a mailbox that never delivers is reported to.
struct Schedule { int refresh; const uint32_t* ready; uint32_t* fault; };

// One pass of the launch chain (run_chain), as the path gets it.  The path fills its arguments, launches, and says what it queued
// where that is not one launch of k steps (chunked launches; a graph replay consumes ten launches' worth).
struct ChainStep {
  int k;                  // world steps of this launch: min(per_launch, left)
  int left;               // steps of the call not yet queued, this launch's included
  uint32_t first_flag;    // kFlagFirstWorldStep at the first world step since Load, else 0
  uint64_t publish_mask;  // which of the k steps publish (bit j: world step h->step + j)
  void* record;           // where this launch's first observable image goes, null without a record
  int used, launches;     // out: world steps consumed, launches queued (k and 1 unless the path says otherwise)
};

// One observable image: fp32 handles n_obs float4 slot rows, precision = 64 handles f64_obs_rows(n) rows of doubles
inline size_t image_bytes(const cdpr_engine* h) {
  return h->plan.fp64 ? (size_t)f64_obs_rows((int)h->n) * h->stride * sizeof(double) : (size_t)h->n_obs * h->stride * sizeof(float4);
}

// cdpr_engine.hip
int set_device(cdpr_engine* h);
int drain_copy_stream(cdpr_engine* h);
int check_fault(cdpr_engine* h);
int checked(cdpr_engine* h, int rc);
std::vector<float4> home_state(const cdpr_engine* h, uint32_t rows);
// cdpr_engine_launch.hip
double sim_time(uint64_t step, double dt);
LaunchShape launch_shape(const cdpr_engine* h, int k, bool steady = false, const Schedule* sched = nullptr);
int refuse_missing(cdpr_engine* h, const PlannedKernel& missing);  // CDPR_ERR_UNSUPPORTED "internal: no instantiation for <label>", or CDPR_OK for id None
int warm_first_launch(cdpr_engine* h);
uint64_t publish_mask(const cdpr_engine* h, int k, double& last);  // which of the next k world steps publish; `last`: the publish stamp after them
void advance_clock(cdpr_engine* h, int k, int launches);            // k world steps were queued in `launches` launches
int run_steps(cdpr_engine* h, int nsteps, int per_launch, void* record = nullptr, const Schedule* sched = nullptr);
int scheduled_update(cdpr_engine* h, uint32_t kind, int nsteps, int refresh_steps, const float* d_commands, const uint32_t* d_ready, const uint8_t* d_masks,
                     void* d_record, size_t record_bytes);
// cdpr_engine_reset.hip
int launch_reset(cdpr_engine* h, const uint8_t* d_mask, const float* d_pose, const float* d_twist);
// cdpr_engine_copy.hip
int launch_copy(cdpr_engine* h, const int32_t* d_source, uint32_t* d_status, bool zeroed = false);
// cdpr_engine_done.hip
int done_checks(cdpr_engine* h, const cdpr_done_rule_t* rule, const char* what);  // what every call refuses of a done rule
int ensure_done_scratch(cdpr_engine* h);                                          // h->d_done: [mask | reason | counts]
// cdpr_engine_f64.hip
int build_f64(cdpr_engine* h);  // cdpr_create's part of a precision = 64 handle
size_t state64_rows(const cdpr_engine* h);
int upload_home64(cdpr_engine* h);
int run_steps_f64(cdpr_engine* h, int nsteps, int per_launch, bool reset_pid, void* record, const PlannedKernel& pk1, const PlannedKernel& pkk);  // (its path of the chain; run_steps has latched the commands)
int rollout_enqueue_f64(cdpr_engine* h, int samples, int horizon, const float* d_commands, const float* d_ref, float* d_cost);

// The handle as the kernels that act on chosen robots see it (cdpr_robot_records.hpp), one builder per record layout: the only
// places that say where a robot's records are.
inline PlatRows plat_rows(const cdpr_engine* h) {
  return PlatRows{h->d_state, h->d_obs, h->dbg ? h->d_dbg.p : nullptr, h->stride, (uint32_t)h->n_state, (uint32_t)h->n_obs, h->plan.fk ? 1u : 0u};
}
inline FastRecords fast_records(const cdpr_engine* h) {
  FastRecords v{};
  v.plat = plat_rows(h);
  v.integral = h->d_state + (size_t)(plat_slots(h->plan.fk) + 5 * cable_pairs((int)h->n)) * h->stride;
  v.integral_rows = (uint32_t)((cable_pairs((int)h->n) + 1) / 2);
  v.meta = h->d_mode, v.target = h->d_target, v.episode_start = h->d_episode;
  v.batch = h->batch, v.n = h->n;
  return v;
}
inline GenRecords gen_records(const cdpr_engine* h) {
  GenRecords v{};
  v.plat = plat_rows(h);
  v.rec = h->d_rec, v.lay = h->args.glay;
  v.mode = h->d_mode, v.episode_start = h->d_episode;
  for (int k = 0; k < kCmdKinds; ++k) v.latched[k] = h->cmd[k].d[0];
  v.batch = h->batch, v.n = h->n;
  return v;
}
inline F64Records f64_records(const cdpr_engine* h) {
  F64Records v{};
  v.state = h->d_state64, v.obs = h->d_obs64, v.dbg = h->d_dbg64;
  v.meta = h->d_mode, v.target = h->d_target, v.episode_start = h->d_episode;
  v.stride = h->stride, v.state_rows = (uint32_t)state64_rows(h), v.obs_rows = (uint32_t)f64_obs_rows((int)h->n);
  v.batch = h->batch, v.n = h->n;
  v.hold = h->plan.hold64 ? 1u : 0u, v.hold_win = (uint32_t)hold_win(h->plan), v.win = (uint32_t)win64(h->plan);
  for (int c = 0; c < 7; ++c) v.home[c] = h->cfg.home_pose[c];
  return v;
}

// one thread per robot, 256 per block (the latch, reset, copy and verdict kernels)
constexpr uint32_t kRobotBlock = 256u;
inline dim3 robot_grid(const cdpr_engine* h) { return dim3((h->batch + kRobotBlock - 1u) / kRobotBlock); }

// `who` over the robots of a per-robot handle, on the handle's stream: one launch of the kernel of the handle's record layout.
// settle_commands: the launch writes rows of the general path's LATCHED command buffers from outside a latch (a model reset, a
// copy): whatever the copy stream still carries has landed first, as in front of the masked setters.
template <typename Who, typename KFast, typename KGen, typename KF64>
int launch_per_robot(cdpr_engine* h, const Who& who, KFast fast, KGen gen, KF64 f64, bool settle_commands) {
  const dim3 grid = robot_grid(h), block(kRobotBlock);
  if (h->plan.fp64) {
    hipLaunchKernelGGL(f64, grid, block, 0, h->stream, who, f64_records(h));
  } else if (!h->plan.general) {
    hipLaunchKernelGGL(fast, grid, block, 0, h->stream, who, fast_records(h));
  } else {
    if (settle_commands)
      if (int rc = drain_copy_stream(h)) return rc;
    hipLaunchKernelGGL(gen, grid, block, 0, h->stream, who, gen_records(h));
  }
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

// counts a verdict kernel adds to (cdpr_done.hpp, copy_verdict): zeroed on the stream in front of the launch; null: none wanted
inline int zero_counts(cdpr_engine* h, uint32_t* d_counts, size_t count) {
  if (d_counts) HIP_TRY(h, hipMemsetAsync(d_counts, 0, count * sizeof(uint32_t), h->stream));
  return CDPR_OK;
}

// What every call that acts on chosen robots refuses: a uniform handle (it keeps ONE mode and one Pid call count for the whole
// batch), and `missing`, the name of a required argument that came as null.
inline int per_robot_checks(cdpr_engine* h, const char* what, const char* missing = nullptr) {
  if (!h->plan.per_robot) {
    h->err = std::string(what) + " needs a handle created with per_robot_commands = 1";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (missing) {
    h->err = std::string(what) + ": null " + missing;
    return CDPR_ERR_INVALID;
  }
  return CDPR_OK;
}

// The loop every path runs (fp32 and general: cdpr_engine_launch.hip, precision = 64: cdpr_engine_f64.hip): the steps of this launch,
// the first-world-step flag, the record moved on by the images done, the publish mask; then the path fills and launches (`path`:
// int(ChainStep&), an error code), the clock moves by what it consumed, and after the last launch the latest recorded image goes
// into the handle's own observables (own_obs), which cdpr_get_* read.
template <typename Path>
int run_chain(cdpr_engine* h, int nsteps, int per_launch, void* record, void* own_obs, Path&& path) {
  const size_t image = image_bytes(h);
  int done = 0;
  while (done < nsteps) {
    ChainStep s{};
    s.k = s.used = std::min(per_launch, nsteps - done);
    s.left = nsteps - done;
    s.launches = 1;
    s.first_flag = (steps_since_load(h) == 0) ? kFlagFirstWorldStep : 0u;
    s.record = record ? static_cast<char*>(record) + (size_t)done * image : nullptr;
    double last;
    s.publish_mask = publish_mask(h, s.k, last);
    if (int rc = path(s)) return rc;
    advance_clock(h, s.used, s.launches);
    done += s.used;
  }
  if (record && h->cfg.publish_period == 0.0 && steps_since_load(h) > 1)  // keep cdpr_get_* consistent: latest image into the engine's own
    HIP_TRY(h, hipMemcpyAsync(own_obs, static_cast<char*>(record) + (size_t)(nsteps - 1) * image, image, hipMemcpyDeviceToDevice, h->stream));
  return CDPR_OK;
}

}  // namespace cdpr_host
