// cdpr_engine_done.hip - cdpr_evaluate_done / cdpr_evaluate_done_device / cdpr_reset_done_device / cdpr_get_episode_start: the verdict of
// a done rule, one launch of the kernel of the handle's platform layout (cdpr_done.hpp) on the handle's stream, and the episode
// clock's read-out.  The device forms neither wait for the stream nor copy anything back.  These are not step launches: h->last_kernel
// and the launch counter stay as the last step left them.
#include "cdpr_engine_internal.hpp"
#include "cdpr_done.hpp"

namespace cdpr_host {

// (also what cdpr_env_evaluate_device refuses of its spec's rule: cdpr_engine_env.hip)
int done_checks(cdpr_engine* h, const cdpr_done_rule_t* rule, const char* what) {
  if (!rule) {
    h->err = std::string(what) + ": null rule";
    return CDPR_ERR_INVALID;
  }
  if (rule->struct_size != sizeof(cdpr_done_rule_t)) {
    h->err = std::string(what) + ": rule.struct_size is not sizeof(cdpr_done_rule_t)";
    return CDPR_ERR_INVALID;
  }
  if ((rule->enable & CDPR_DONE_FK_RESIDUAL) && !h->plan.fk) {
    h->err = std::string(what) + ": CDPR_DONE_FK_RESIDUAL needs CDPR_STAGE_FK";
    return CDPR_ERR_UNSUPPORTED;
  }
  if ((rule->enable & CDPR_DONE_INFEASIBLE) && !h->plan.td) {
    h->err = std::string(what) + ": CDPR_DONE_INFEASIBLE needs CDPR_STAGE_TD";
    return CDPR_ERR_UNSUPPORTED;
  }
  return CDPR_OK;
}

// the handle's own [mask | reason | counts] block (cdpr_engine::d_done)
struct DoneScratch {
  size_t off_reason, off_counts, bytes;
  explicit DoneScratch(size_t B) : off_reason((B + 15u) & ~(size_t)15u), off_counts(off_reason + B * sizeof(uint32_t)), bytes(off_counts + CDPR_DONE_COUNTS * sizeof(uint32_t)) {}
};

// ... allocated at its first use; its mask also serves cdpr_env_evaluate_device where the caller wants a reason or counts without one
int ensure_done_scratch(cdpr_engine* h) {
  if (!h->d_done) HIP_TRY(h, h->d_done.alloc(DoneScratch(h->batch).bytes));
  return CDPR_OK;
}

// Queue the verdict behind every update queued so far: d_mask uint8[B], d_reason uint32[B] or null, d_counts uint32[CDPR_DONE_COUNTS]
// or null (zeroed on the stream first).  The step count goes in by value, as into the step kernels.
static int launch_done(cdpr_engine* h, const cdpr_done_rule_t& rule, uint8_t* d_mask, uint32_t* d_reason, uint32_t* d_counts) {
  if (int rc = zero_counts(h, d_counts, CDPR_DONE_COUNTS)) return rc;
  const dim3 grid = robot_grid(h), block(kRobotBlock);
  DoneOut out{};
  out.mask = d_mask, out.reason = d_reason, out.counts = d_counts;
  if (h->plan.fp64) {
    DoneF64Args a{};
    a.rule = rule;
    a.state = h->d_state64, a.obs = h->d_obs64, a.episode_start = h->d_episode;
    a.stride = h->stride, a.batch = h->batch, a.step = (uint32_t)h->step;
    a.out = out;
    hipLaunchKernelGGL(cdpr_done_f64_kernel, grid, block, 0, h->stream, a);
  } else {
    DoneArgs a{};
    a.rule = rule;
    a.state = h->d_state, a.obs = h->d_obs, a.episode_start = h->d_episode;
    a.stride = h->stride, a.batch = h->batch, a.step = (uint32_t)h->step;
    a.out = out;
    hipLaunchKernelGGL(cdpr_done_kernel, grid, block, 0, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // namespace cdpr_host

extern "C" {

size_t cdpr_done_rule_size(void) { return sizeof(cdpr_done_rule_t); }

int cdpr_evaluate_done_device(cdpr_handle_t h, const cdpr_done_rule_t* rule, uint8_t* d_mask, uint32_t* d_reason, uint32_t* d_counts) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = done_checks(h, rule, "cdpr_evaluate_done_device")) return rc;
  if (!d_mask) {
    h->err = "cdpr_evaluate_done_device: null robot mask";
    return CDPR_ERR_INVALID;
  }
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_done(h, *rule, d_mask, d_reason, d_counts);
}

int cdpr_evaluate_done(cdpr_handle_t h, const cdpr_done_rule_t* rule, uint8_t* mask, uint32_t* reason, uint32_t* counts) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = done_checks(h, rule, "cdpr_evaluate_done")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  const size_t B = h->batch;
  const DoneScratch s(B);
  if (int rc = ensure_done_scratch(h)) return rc;
  char* const d = h->d_done;
  if (int rc = launch_done(h, *rule, reinterpret_cast<uint8_t*>(d), reinterpret_cast<uint32_t*>(d + s.off_reason), reinterpret_cast<uint32_t*>(d + s.off_counts))) return rc;
  if (mask) HIP_TRY(h, hipMemcpyAsync(mask, d, B, hipMemcpyDeviceToHost, h->stream));
  if (reason) HIP_TRY(h, hipMemcpyAsync(reason, d + s.off_reason, B * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (counts) HIP_TRY(h, hipMemcpyAsync(counts, d + s.off_counts, CDPR_DONE_COUNTS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, wait_stream(h));
  return check_fault(h);
}

int cdpr_reset_done_device(cdpr_handle_t h, const cdpr_done_rule_t* rule, const float* d_pose7, const float* d_twist6, uint32_t* d_counts) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = done_checks(h, rule, "cdpr_reset_done_device")) return rc;
  if (int rc = per_robot_checks(h, "cdpr_reset_done_device")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (int rc = ensure_done_scratch(h)) return rc;
  uint8_t* const d_mask = reinterpret_cast<uint8_t*>(h->d_done.p);
  if (int rc = launch_done(h, *rule, d_mask, nullptr, d_counts)) return rc;
  return launch_reset(h, d_mask, d_pose7, d_twist6);  // stream-ordered behind the verdict: no host wait in between
}

int cdpr_get_episode_start(cdpr_handle_t h, uint32_t* start) {
  if (!h || !start) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  HIP_TRY(h, hipMemcpyAsync(start, h->d_episode, (size_t)h->batch * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, wait_stream(h));
  return check_fault(h);
}

}  // extern "C"
