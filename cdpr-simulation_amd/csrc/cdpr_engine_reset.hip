// cdpr_engine_reset.hip - cdpr_reset_robots / cdpr_reset_robots_device: the model reset of chosen robots of a per-robot handle, one
// launch of the reset kernel of the handle's record layout (cdpr_reset.hpp) on the handle's stream.  Neither form waits for the
// stream or copies anything back.  Reference paths as in cdpr_engine.hip.
#include "cdpr_engine_internal.hpp"
#include "cdpr_reset.hpp"

namespace cdpr_host {

static int reset_checks(cdpr_engine* h, const void* mask, const char* what) {
  if (!h->plan.per_robot) {  // (a uniform handle keeps ONE mode and one Pid call count for the whole batch)
    h->err = std::string(what) + " needs a handle created with per_robot_commands = 1";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (!mask) {
    h->err = std::string(what) + ": null robot mask";
    return CDPR_ERR_INVALID;
  }
  return CDPR_OK;
}

// Queue the reset behind every update queued so far.  d_mask uint8[B], d_pose float[B][7] or null (home), d_twist float[B][6] or null
// (zero): device buffers.  h->mode, h->pid_calls (not used on per-robot handles), the world step, the publish clock, the status word
// and every pending command stay as they are; the reset robots' episode clock takes the world step of the call.  (Also the second
// launch of cdpr_reset_done_device, cdpr_engine_done.hip.)
int launch_reset(cdpr_engine* h, const uint8_t* d_mask, const float* d_pose, const float* d_twist) {
  ResetWhere who{};
  who.mask = d_mask, who.pose = d_pose, who.twist = d_twist, who.batch = h->batch;
  who.episode_start = h->d_episode, who.step = (uint32_t)h->step;
  for (int c = 0; c < 7; ++c) who.home[c] = (float)h->cfg.home_pose[c];
  const dim3 grid((h->batch + 255u) / 256u), block(256);
  if (h->plan.fp64) {
    ResetF64Args a{};
    a.who = who;
    for (int c = 0; c < 7; ++c) a.home[c] = h->cfg.home_pose[c];
    a.state = h->d_state64, a.obs = h->d_obs64, a.dbg = h->d_dbg64;
    a.meta = h->d_mode, a.target = h->d_target;
    a.stride = h->stride, a.n = h->n;
    a.hold = h->plan.hold64 ? 1u : 0u, a.hold_win = (uint32_t)hold_win(h), a.win = (uint32_t)win64(h);
    hipLaunchKernelGGL(cdpr_reset_f64_kernel, grid, block, 0, h->stream, a);
  } else {
    ResetPlatform plat{};
    plat.state = h->d_state, plat.obs = h->d_obs, plat.dbg = h->dbg ? h->d_dbg.p : nullptr;
    plat.stride = h->stride, plat.n_obs = (uint32_t)h->n_obs, plat.fk = h->plan.fk ? 1u : 0u;
    if (!h->plan.general) {
      ResetFastArgs a{};
      a.who = who, a.plat = plat;
      a.meta = h->d_mode, a.target = h->d_target;
      a.hot = h->d_state + (size_t)(plat_slots(h->plan.fk) + 5 * cable_pairs((int)h->n)) * h->stride;
      a.n = h->n, a.hot_rows = (uint32_t)((cable_pairs((int)h->n) + 1) / 2);
      hipLaunchKernelGGL(cdpr_reset_fast_kernel, grid, block, 0, h->stream, a);
    } else {
      // the launch writes the robots' rows of the LATCHED command buffers: whatever the copy stream still carries has landed first,
      // as in front of the masked setters.  (No flush_hot: that would take every steady robot out of its hot rows for nbuf steps to
      // reset a handful; the reset robot's own word is cleared with its records.)
      if (int rc = drain_copy_stream(h)) return rc;
      ResetGenArgs a{};
      a.who = who, a.plat = plat;
      a.mode = h->d_mode;
      for (int k = 0; k < kCmdKinds; ++k) a.latched[k] = h->cmd[k].d[0];
      a.rec = h->d_rec, a.rstride = h->stride, a.n = h->n, a.lay = h->glay;
      hipLaunchKernelGGL(cdpr_reset_gen_kernel, grid, block, 0, h->stream, a);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // namespace cdpr_host

extern "C" {

int cdpr_reset_robots_device(cdpr_handle_t h, const uint8_t* d_robot_mask, const float* d_pose7, const float* d_twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = reset_checks(h, d_robot_mask, "cdpr_reset_robots_device")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_reset(h, d_robot_mask, d_pose7, d_twist6);
}

int cdpr_reset_robots(cdpr_handle_t h, const uint8_t* robot_mask, const float* pose7, const float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = reset_checks(h, robot_mask, "cdpr_reset_robots")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  // [mask, padded to 16 B | pose | twist]: into a pinned block (the caller may reuse its arrays on return), from there to the device
  // scratch on the handle's stream.  Two blocks take turns: the one filled now was last read by the copy of two calls back.
  const size_t B = h->batch, off_pose = (B + 15u) & ~(size_t)15u, off_twist = off_pose + B * 7 * sizeof(float), bytes = off_twist + B * 6 * sizeof(float);
  if (!h->d_reset_args) HIP_TRY(h, h->d_reset_args.alloc(bytes));
  const int idx = (h->reset_idx ^= 1);
  if (!h->h_reset_stage[idx]) HIP_TRY(h, h->h_reset_stage[idx].alloc(bytes, hipHostMallocDefault));
  if (!h->reset_ev[idx]) HIP_TRY(h, hipEventCreateWithFlags(&h->reset_ev[idx], hipEventDisableTiming));
  if (h->reset_ev_set[idx]) HIP_TRY(h, hipEventSynchronize(h->reset_ev[idx]));
  char* const stage = h->h_reset_stage[idx];
  memcpy(stage, robot_mask, B);
  if (pose7) memcpy(stage + off_pose, pose7, B * 7 * sizeof(float));
  if (twist6) memcpy(stage + off_twist, twist6, B * 6 * sizeof(float));
  HIP_TRY(h, hipMemcpyAsync(h->d_reset_args, stage, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->reset_ev[idx], h->stream));
  h->reset_ev_set[idx] = true;
  char* const d = h->d_reset_args;
  return launch_reset(h, reinterpret_cast<const uint8_t*>(d), pose7 ? reinterpret_cast<const float*>(d + off_pose) : nullptr,
                      twist6 ? reinterpret_cast<const float*>(d + off_twist) : nullptr);
}

}  // extern "C"
