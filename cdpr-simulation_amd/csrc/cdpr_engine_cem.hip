// cdpr_engine_cem.hip - cdpr_cem_sample_device / cdpr_cem_update_device / cdpr_cem_spec_size: the cross-entropy method around
// cdpr_rollout_velocity_device, beside MPPI (cdpr_engine_mppi.hip) - the command batch from a mean and a sigma plan, both plans refitted
// to the K best samples (cdpr_cem.hpp, instantiated in k_cem.hip).  One launch each on the handle's stream; neither waits for the
// stream, copies anything back or reads robot state: the handle supplies B, n and the stream.  Not step launches: h->last_kernel and
// the launch counter stay as they are.
#include "cdpr_engine_internal.hpp"
#include "cdpr_cem.hpp"

namespace cdpr_host {

// what both calls refuse of a spec (the update's alpha and sigma range are plain numbers to the sampler too: one rule for both)
static int cem_checks(cdpr_engine* h, const cdpr_cem_spec_t* spec, const char* what) {
  const char* bad = nullptr;
  if (!spec) bad = "null spec";
  else if (spec->struct_size != sizeof(cdpr_cem_spec_t)) bad = "spec.struct_size is not sizeof(cdpr_cem_spec_t)";
  else if (spec->flags & ~(CDPR_CEM_NOMINAL_FIRST | CDPR_CEM_CLAMP | CDPR_CEM_SHIFT)) bad = "unknown bit in spec.flags";
  else if (spec->reserved[0] != 0u || spec->reserved[1] != 0u || spec->reserved[2] != 0u) bad = "spec.reserved must be 0";
  else if (spec->samples == 0u || spec->horizon == 0u || spec->elites == 0u) bad = "spec.samples, spec.horizon and spec.elites must be at least 1";
  else if (spec->elites > spec->samples) bad = "spec.elites passes spec.samples";
  else if (!(spec->alpha > 0.0f && spec->alpha <= 1.0f)) bad = "spec.alpha is not in (0, 1]";
  else if (!(spec->sigma_min >= 0.0f) || !std::isfinite(spec->sigma_min) || !(spec->sigma_min <= spec->sigma_max))
    bad = "spec.sigma_min is negative, not finite or above spec.sigma_max (or that is a NaN)";
  else if ((spec->flags & CDPR_CEM_CLAMP) && (!std::isfinite(spec->cmd_min) || !std::isfinite(spec->cmd_max) || !(spec->cmd_min <= spec->cmd_max)))
    bad = "CDPR_CEM_CLAMP with bounds that are not finite or cmd_min > cmd_max";
  if (bad) {
    h->err = std::string(what) + ": " + bad;
    return CDPR_ERR_INVALID;
  }
  const uint64_t E = (uint64_t)spec->horizon * (uint64_t)spec->samples;  // (< 2^64: two 32-bit factors; times n <= 12 only after the test)
  if (E > kMppiMaxElems || E * h->n > kMppiMaxElems) {
    h->err = std::string(what) + ": horizon * samples * n passes 2^34 elements per robot";
    return CDPR_ERR_UNSUPPORTED;
  }
  if ((uint64_t)h->batch * (uint64_t)spec->samples > kMppiMaxTraj) {
    h->err = std::string(what) + ": batch * samples passes 2^30 trajectories";
    return CDPR_ERR_UNSUPPORTED;
  }
  return CDPR_OK;
}

static int cem_refuse_null(cdpr_engine* h, const char* what, const char* name) {
  h->err = std::string(what) + ": null " + name;
  return CDPR_ERR_INVALID;
}

}  // namespace cdpr_host

extern "C" {

size_t cdpr_cem_spec_size(void) { return sizeof(cdpr_cem_spec_t); }

int cdpr_cem_sample_device(cdpr_handle_t h, const cdpr_cem_spec_t* spec, uint32_t iteration, const float* d_mean, const float* d_sigma,
                           float* d_commands) {
  const char* const what = "cdpr_cem_sample_device";
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = cem_checks(h, spec, what)) return rc;
  if (!d_mean) return cem_refuse_null(h, what, "mean plan");
  if (!d_sigma) return cem_refuse_null(h, what, "sigma plan");
  if (!d_commands) return cem_refuse_null(h, what, "command buffer");
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  MppiSampleArgs a{};
  a.nominal = d_mean, a.sigma_plan = d_sigma, a.commands = d_commands;
  const dim3 grid = mppi_sample_geometry(a, h->batch, spec->samples, spec->horizon, h->n);
  a.flags = spec->flags, a.lo = spec->cmd_min, a.hi = spec->cmd_max;  // (the flag bits are MPPI's)
  a.key0 = spec->seed_lo, a.key1 = spec->seed_hi, a.iteration = iteration, a.robot_offset = spec->robot_offset;
  hipLaunchKernelGGL(cem_sample_kernel_entry(mppi_sample_vec(a.elems, d_commands)), grid, dim3(kMppiBlock), 0, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

int cdpr_cem_update_device(cdpr_handle_t h, const cdpr_cem_spec_t* spec, const float* d_cost, const float* d_commands, float* d_mean,
                           float* d_sigma, float* d_action, float* d_elite, int32_t* d_best, uint32_t* d_status) {
  const char* const what = "cdpr_cem_update_device";
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = cem_checks(h, spec, what)) return rc;
  if (!d_cost) return cem_refuse_null(h, what, "cost buffer");
  if (!d_commands) return cem_refuse_null(h, what, "command buffer");
  if (!d_mean) return cem_refuse_null(h, what, "mean plan");
  if (!d_sigma) return cem_refuse_null(h, what, "sigma plan");
  const CemUpdateKernel kernel = cem_update_kernel_entry(h->n);
  if (!kernel) {
    h->err = std::string(what) + ": internal: no instantiation for this cable count";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (int rc = zero_counts(h, d_status, 4)) return rc;
  CemUpdateArgs a{};
  a.cost = d_cost, a.commands = d_commands, a.mean = d_mean, a.sigma = d_sigma;
  a.action = d_action, a.elite = d_elite, a.best = d_best, a.status = d_status;
  a.batch = h->batch, a.samples = spec->samples, a.horizon = spec->horizon, a.elites = spec->elites;
  a.shift = (spec->flags & CDPR_CEM_SHIFT) ? 1u : 0u;
  a.lds_samples = spec->samples <= kCemLdsSamples ? spec->samples : 0u;
  a.vec = (h->n % 4u == 0u && reinterpret_cast<uintptr_t>(d_commands) % 16u == 0u) ? 1u : 0u;
  a.alpha = spec->alpha, a.sigma_min = spec->sigma_min, a.sigma_max = spec->sigma_max;
  hipLaunchKernelGGL(kernel, dim3(h->batch), dim3(kMppiBlock), (size_t)a.lds_samples * 2u * sizeof(uint32_t), h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // extern "C"
