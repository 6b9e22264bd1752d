// cdpr_engine_copy.hip - cdpr_copy_robots / cdpr_copy_robots_device: robots of a per-robot handle continue from where other robots of
// the same handle are now, one launch of the copy kernel of the handle's record layout (cdpr_copy.hpp) on the handle's stream.  Neither
// form waits for the stream or copies anything back.  Not a step launch: h->last_kernel and the launch counter stay as they are.
#include "cdpr_engine_internal.hpp"
#include "cdpr_copy.hpp"

namespace cdpr_host {

static int copy_checks(cdpr_engine* h, const void* source, const char* what) {
  if (!h->plan.per_robot) {  // (as cdpr_reset_robots: a uniform handle keeps ONE mode and one Pid call count for the whole batch)
    h->err = std::string(what) + " needs a handle created with per_robot_commands = 1";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (!source) {
    h->err = std::string(what) + ": null source map";
    return CDPR_ERR_INVALID;
  }
  return CDPR_OK;
}

// Queue the copy behind every update queued so far.  d_source int32[B], d_status uint32[2] or null (zeroed on the stream first):
// device buffers.  The world step, the publish clock, the status word and every pending command stay as they are.
static int launch_copy(cdpr_engine* h, const int32_t* d_source, uint32_t* d_status) {
  if (d_status) HIP_TRY(h, hipMemsetAsync(d_status, 0, 2 * sizeof(uint32_t), h->stream));
  CopyWho who{};
  who.source = d_source, who.status = d_status, who.episode_start = h->d_episode, who.batch = h->batch;
  const dim3 grid((h->batch + 255u) / 256u), block(256);
  if (h->plan.fp64) {
    CopyF64Args a{};
    a.who = who;
    a.state = h->d_state64, a.obs = h->d_obs64, a.dbg = h->d_dbg64;
    a.meta = h->d_mode, a.target = h->d_target;
    a.stride = h->stride, a.n = h->n;
    a.state_rows = (uint32_t)state64_rows(h), a.obs_rows = (uint32_t)f64_obs_rows((int)h->n);
    hipLaunchKernelGGL(cdpr_copy_f64_kernel, grid, block, 0, h->stream, a);
  } else if (!h->plan.general) {
    CopyFastArgs a{};
    a.who = who;
    a.state = h->d_state, a.obs = h->d_obs, a.dbg = h->dbg ? h->d_dbg.p : nullptr;
    a.meta = h->d_mode, a.target = h->d_target;
    a.stride = h->stride, a.n_state = (uint32_t)h->n_state, a.n_obs = (uint32_t)h->n_obs, a.n = h->n;
    hipLaunchKernelGGL(cdpr_copy_fast_kernel, grid, block, 0, h->stream, a);
  } else {
    // the launch writes the destinations' rows of the LATCHED command buffers: whatever the copy stream still carries has landed
    // first, as in front of the reset (launch_reset).  No flush_hot: the hot rows travel as they are.
    if (int rc = drain_copy_stream(h)) return rc;
    CopyGenArgs a{};
    a.who = who;
    a.state = h->d_state, a.obs = h->d_obs, a.dbg = h->dbg ? h->d_dbg.p : nullptr;
    a.mode = h->d_mode;
    for (int k = 0; k < kCmdKinds; ++k) a.latched[k] = h->cmd[k].d[0];
    a.rec = h->d_rec, a.lay = h->glay;
    a.stride = h->stride, a.n_state = (uint32_t)h->n_state, a.n_obs = (uint32_t)h->n_obs, a.n = h->n;
    hipLaunchKernelGGL(cdpr_copy_gen_kernel, grid, block, 0, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // namespace cdpr_host

extern "C" {

int cdpr_copy_robots_device(cdpr_handle_t h, const int32_t* d_source, uint32_t* d_status) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = copy_checks(h, d_source, "cdpr_copy_robots_device")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_copy(h, d_source, d_status);
}

int cdpr_copy_robots(cdpr_handle_t h, const int32_t* source) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = copy_checks(h, source, "cdpr_copy_robots")) return rc;
  // the whole map is judged before anything is queued: what the device form would skip, the host form refuses
  const size_t B = h->batch;
  for (size_t r = 0; r < B; ++r) {
    const int32_t s = source[r];
    if (s < 0 || (size_t)s == r) continue;
    if ((size_t)s >= B) {
      h->err = "cdpr_copy_robots: source[" + std::to_string(r) + "] = " + std::to_string(s) + " is not a robot of this handle";
      return CDPR_ERR_INVALID;
    }
    if (source[s] >= 0 && source[s] != s) {
      h->err = "cdpr_copy_robots: source[" + std::to_string(r) + "] = " + std::to_string(s) + " is itself a destination (a source must be left as it is)";
      return CDPR_ERR_INVALID;
    }
  }
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  // into a pinned block (the caller may reuse its array on return), from there to the device scratch on the handle's stream.  Two
  // blocks take turns: the one filled now was last read by the copy of two calls back (as cdpr_reset_robots stages its arguments).
  const size_t bytes = B * sizeof(int32_t);
  if (!h->d_copy_map) HIP_TRY(h, h->d_copy_map.alloc(bytes));
  const int idx = (h->copy_idx ^= 1);
  if (!h->h_copy_stage[idx]) HIP_TRY(h, h->h_copy_stage[idx].alloc(bytes, hipHostMallocDefault));
  if (!h->copy_ev[idx]) HIP_TRY(h, hipEventCreateWithFlags(&h->copy_ev[idx], hipEventDisableTiming));
  if (h->copy_ev_set[idx]) HIP_TRY(h, hipEventSynchronize(h->copy_ev[idx]));
  memcpy(h->h_copy_stage[idx], source, bytes);
  HIP_TRY(h, hipMemcpyAsync(h->d_copy_map, h->h_copy_stage[idx], bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->copy_ev[idx], h->stream));
  h->copy_ev_set[idx] = true;
  return launch_copy(h, h->d_copy_map, nullptr);
}

}  // extern "C"
