// cdpr_engine_env.hip - cdpr_observe_device / cdpr_env_evaluate_device / cdpr_observation_width / cdpr_env_spec_size: the environment
// view, one launch of the kernel of the handle's platform layout (cdpr_env.hpp, instantiated in k_env.hip) on the handle's stream.
// Neither call waits for the stream or copies anything back.  These are not step launches: h->last_kernel and the launch counter stay
// as the last step left them.
#include "cdpr_engine_internal.hpp"
#include "cdpr_env.hpp"

namespace cdpr_host {

// the packed width of `fields` on n cables, and - `col` - the field table: the first column of every field bit, in bit order
static uint32_t env_columns(uint32_t fields, uint32_t n, uint8_t* col) {
  uint32_t width = 0;
  for (int k = 0; k < kEnvFields; ++k) {
    if (col) col[k] = (uint8_t)width;
    if ((fields >> k) & 1u) width += env_field_width(k, n);
  }
  return width;
}

// what both calls refuse of an observation request (`wanted`: a tensor is given); ld becomes the row length in floats
static int obs_checks(cdpr_engine* h, uint32_t fields, uint32_t& ld, bool wanted, const char* what) {
  if (fields & ~kEnvKnownFields) {
    h->err = std::string(what) + ": unknown CDPR_OBS_* bit";
    return CDPR_ERR_INVALID;
  }
  if (wanted && fields == 0u) {
    h->err = std::string(what) + ": an observation tensor with no fields";
    return CDPR_ERR_INVALID;
  }
  const uint32_t width = env_columns(fields, h->n, nullptr);
  if (ld != 0u && ld < width) {
    h->err = std::string(what) + ": ld is below the width of the fields";
    return CDPR_ERR_INVALID;
  }
  if ((fields & kEnvFkFields) && !h->plan.fk) {
    h->err = std::string(what) + ": CDPR_OBS_FK_POSE / CDPR_OBS_FK_RESIDUAL need CDPR_STAGE_FK";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (ld == 0u) ld = width;
  return CDPR_OK;
}

// Queue the view behind every update queued so far.  v: rule, weights, target and outputs as the caller gave them; the rest is filled
// here.  The step count goes in by value, as into the step kernels.
static int launch_env(cdpr_engine* h, EnvView v, uint32_t fields, uint32_t ld) {
  if (int rc = zero_counts(h, v.out.counts, CDPR_DONE_COUNTS)) return rc;
  v.fields = v.obs ? fields : 0u;
  v.width = env_columns(v.fields, h->n, v.col);
  v.ld = ld;
  for (int c = 0; c < 7; ++c) v.home[c] = (float)h->cfg.home_pose[c];
  v.episode_start = h->d_episode;
  v.stride = h->stride, v.batch = h->batch, v.n = h->n, v.step = (uint32_t)h->step;
  const dim3 grid((h->batch + (uint32_t)kEnvBlock - 1u) / (uint32_t)kEnvBlock), block(kEnvBlock);
  const size_t lds = v.obs ? env_lds_bytes(v.width) : 0;
  if (h->plan.fp64) {
    EnvF64Args a{};
    a.view = v, a.state = h->d_state64, a.obs_rows = h->d_obs64;
    hipLaunchKernelGGL(pick_env_f64_kernel(), grid, block, lds, h->stream, a);
  } else {
    EnvArgs a{};
    a.view = v, a.state = h->d_state, a.obs_rows = h->d_obs;
    hipLaunchKernelGGL(pick_env_kernel(), grid, block, lds, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // namespace cdpr_host

extern "C" {

size_t cdpr_env_spec_size(void) { return sizeof(cdpr_env_spec_t); }

int cdpr_observation_width(cdpr_handle_t h, uint32_t fields, uint32_t* width) {
  if (!h) return CDPR_ERR_INVALID;
  if (!width) {
    h->err = "cdpr_observation_width: null width";
    return CDPR_ERR_INVALID;
  }
  if (fields & ~kEnvKnownFields) {
    h->err = "cdpr_observation_width: unknown CDPR_OBS_* bit";
    return CDPR_ERR_INVALID;
  }
  *width = env_columns(fields, h->n, nullptr);
  return CDPR_OK;
}

int cdpr_observe_device(cdpr_handle_t h, uint32_t fields, uint32_t ld, const uint8_t* d_row_mask, float* d_obs) {
  if (!h) return CDPR_ERR_INVALID;
  if (!d_obs) {
    h->err = "cdpr_observe_device: null observation tensor";
    return CDPR_ERR_INVALID;
  }
  if (int rc = obs_checks(h, fields, ld, true, "cdpr_observe_device")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  EnvView v{};
  v.obs = d_obs, v.row_mask = d_row_mask;
  return launch_env(h, v, fields, ld);
}

int cdpr_env_evaluate_device(cdpr_handle_t h, const cdpr_env_spec_t* spec, const float* d_target7, float* d_obs, float* d_reward, uint8_t* d_mask,
                             uint32_t* d_reason, uint32_t* d_counts) {
  const char* const what = "cdpr_env_evaluate_device";
  if (!h) return CDPR_ERR_INVALID;
  if (!spec) {
    h->err = std::string(what) + ": null spec";
    return CDPR_ERR_INVALID;
  }
  if (spec->struct_size != sizeof(cdpr_env_spec_t)) {
    h->err = std::string(what) + ": spec.struct_size is not sizeof(cdpr_env_spec_t)";
    return CDPR_ERR_INVALID;
  }
  if (!d_obs && !d_reward && !d_mask && !d_reason && !d_counts) {
    h->err = std::string(what) + ": every output is null";
    return CDPR_ERR_INVALID;
  }
  uint32_t ld = spec->ld;
  if (int rc = obs_checks(h, spec->fields, ld, d_obs != nullptr, what)) return rc;
  if (spec->w_fk_residual != 0.0f && !h->plan.fk) {
    h->err = std::string(what) + ": w_fk_residual needs CDPR_STAGE_FK";
    return CDPR_ERR_UNSUPPORTED;
  }
  if (int rc = done_checks(h, &spec->done, what)) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  EnvView v{};
  v.rule = spec->done;
  const float w[kEnvWeights] = {spec->w_position, spec->w_orientation, spec->w_speed, spec->w_rate, spec->w_effort, spec->w_fk_residual};
  for (int k = 0; k < kEnvWeights; ++k) v.w[k] = w[k];
  v.alive = spec->alive, v.done_penalty = spec->done_penalty;
  v.target = d_target7;
  v.obs = d_obs, v.reward = d_reward;
  v.out.mask = d_mask, v.out.reason = d_reason, v.out.counts = d_counts;
  if (!d_mask && (d_reason || d_counts)) {  // (done_store writes a mask: the handle's own takes it)
    if (int rc = ensure_done_scratch(h)) return rc;
    v.out.mask = reinterpret_cast<uint8_t*>(h->d_done.p);
  }
  // with no verdict output and nothing enabled the reason word is 0 by definition: no verdict work at all
  v.verdict = (v.out.mask || (d_reward && spec->done.enable != 0u)) ? 1u : 0u;
  return launch_env(h, v, spec->fields, ld);
}

}  // extern "C"
