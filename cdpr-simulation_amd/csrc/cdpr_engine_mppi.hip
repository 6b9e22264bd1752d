// cdpr_engine_mppi.hip - cdpr_mppi_sample_device / cdpr_mppi_update_device / cdpr_mppi_spec_size: the two calls around
// cdpr_rollout_velocity_device that keep an MPPI loop on the GPU - the perturbed command batch from the nominal plan, the rollout's
// costs folded into the next plan and the action to apply (cdpr_mppi.hpp, instantiated in k_mppi.hip).  One launch each on the handle's
// stream; neither waits for the stream, copies anything back or reads robot state: the handle supplies B, n and the stream.  Not step
// launches: h->last_kernel and the launch counter stay as they are.
#include "cdpr_engine_internal.hpp"
#include "cdpr_mppi.hpp"

namespace cdpr_host {

// what both calls refuse of a spec; E becomes H * S * n
static int mppi_checks(cdpr_engine* h, const cdpr_mppi_spec_t* spec, bool update, uint64_t& E, const char* what) {
  const char* bad = nullptr;
  if (!spec) bad = "null spec";
  else if (spec->struct_size != sizeof(cdpr_mppi_spec_t)) bad = "spec.struct_size is not sizeof(cdpr_mppi_spec_t)";
  else if (spec->flags & ~(CDPR_MPPI_NOMINAL_FIRST | CDPR_MPPI_CLAMP | CDPR_MPPI_SHIFT)) bad = "unknown bit in spec.flags";
  else if (spec->reserved != 0u) bad = "spec.reserved must be 0";
  else if (spec->samples == 0u || spec->horizon == 0u) bad = "spec.samples and spec.horizon must be at least 1";
  else if (!(spec->sigma >= 0.0f) || !std::isfinite(spec->sigma)) bad = "spec.sigma is negative or not finite";
  else if (update && (!(spec->temperature > 0.0f) || !std::isfinite(spec->temperature))) bad = "spec.temperature is not finite and > 0";
  else if ((spec->flags & CDPR_MPPI_CLAMP) && (!std::isfinite(spec->cmd_min) || !std::isfinite(spec->cmd_max) || !(spec->cmd_min <= spec->cmd_max)))
    bad = "CDPR_MPPI_CLAMP with bounds that are not finite or cmd_min > cmd_max";
  if (bad) {
    h->err = std::string(what) + ": " + bad;
    return CDPR_ERR_INVALID;
  }
  E = (uint64_t)spec->horizon * (uint64_t)spec->samples;  // (< 2^64: two 32-bit factors; times n <= 12 only after the test below)
  if (E > kMppiMaxElems || E * h->n > kMppiMaxElems) {
    h->err = std::string(what) + ": horizon * samples * n passes 2^34 elements per robot";
    return CDPR_ERR_UNSUPPORTED;
  }
  E *= h->n;
  if ((uint64_t)h->batch * (uint64_t)spec->samples > kMppiMaxTraj) {
    h->err = std::string(what) + ": batch * samples passes 2^30 trajectories";
    return CDPR_ERR_UNSUPPORTED;
  }
  return CDPR_OK;
}

static int refuse_null(cdpr_engine* h, const char* what, const char* name) {
  h->err = std::string(what) + ": null " + name;
  return CDPR_ERR_INVALID;
}

}  // namespace cdpr_host

extern "C" {

size_t cdpr_mppi_spec_size(void) { return sizeof(cdpr_mppi_spec_t); }

int cdpr_mppi_sample_device(cdpr_handle_t h, const cdpr_mppi_spec_t* spec, uint32_t iteration, const float* d_nominal, float* d_commands) {
  const char* const what = "cdpr_mppi_sample_device";
  if (!h) return CDPR_ERR_INVALID;
  uint64_t E = 0;
  if (int rc = mppi_checks(h, spec, false, E, what)) return rc;
  if (!d_nominal) return refuse_null(h, what, "nominal plan");
  if (!d_commands) return refuse_null(h, what, "command buffer");
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  MppiSampleArgs a{};
  a.nominal = d_nominal, a.commands = d_commands;
  const dim3 grid = mppi_sample_geometry(a, h->batch, spec->samples, spec->horizon, h->n);
  a.flags = spec->flags, a.sigma = spec->sigma, a.lo = spec->cmd_min, a.hi = spec->cmd_max;
  a.key0 = spec->seed_lo, a.key1 = spec->seed_hi, a.iteration = iteration, a.robot_offset = spec->robot_offset;
  hipLaunchKernelGGL(mppi_sample_kernel_entry(mppi_sample_vec(E, d_commands)), grid, dim3(kMppiBlock), 0, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

int cdpr_mppi_update_device(cdpr_handle_t h, const cdpr_mppi_spec_t* spec, const float* d_cost, const float* d_commands, float* d_nominal,
                            float* d_action, float* d_weights, float* d_ess, uint32_t* d_status) {
  const char* const what = "cdpr_mppi_update_device";
  if (!h) return CDPR_ERR_INVALID;
  uint64_t E = 0;
  if (int rc = mppi_checks(h, spec, true, E, what)) return rc;
  if (!d_cost) return refuse_null(h, what, "cost buffer");
  if (!d_commands) return refuse_null(h, what, "command buffer");
  if (!d_nominal) return refuse_null(h, what, "nominal plan");
  const MppiUpdateKernel kernel = mppi_update_kernel_entry(h->n);
  if (!kernel) {
    h->err = std::string(what) + ": internal: no instantiation for this cable count";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (int rc = zero_counts(h, d_status, 3)) return rc;
  MppiUpdateArgs a{};
  a.cost = d_cost, a.commands = d_commands, a.nominal = d_nominal, a.action = d_action, a.weights = d_weights, a.ess = d_ess, a.status = d_status;
  a.batch = h->batch, a.samples = spec->samples, a.horizon = spec->horizon;
  a.shift = (spec->flags & CDPR_MPPI_SHIFT) ? 1u : 0u;
  a.lds_samples = spec->samples <= kMppiLdsSamples ? spec->samples : 0u;
  a.vec = (h->n % 4u == 0u && reinterpret_cast<uintptr_t>(d_commands) % 16u == 0u) ? 1u : 0u;
  a.temperature = spec->temperature;
  hipLaunchKernelGGL(kernel, dim3(h->batch), dim3(kMppiBlock), (size_t)a.lds_samples * sizeof(float), h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // extern "C"
