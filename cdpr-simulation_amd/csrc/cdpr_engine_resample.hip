// cdpr_engine_resample.hip - cdpr_resample_map_device / cdpr_resample_device / cdpr_resample_spec_size: systematic resampling per group
// of consecutive robots, float weights to the int32 source map of cdpr_copy_robots_device, one launch of the kernel of the group
// size's form (cdpr_resample.hpp, instantiated in k_resample.hip) on the handle's stream - and, the fused form, the copy kernel of the
// handle's record layout right behind it.  Neither call waits for the stream or copies anything back.  Not step launches:
// h->last_kernel and the launch counter stay as they are.
#include "cdpr_engine_internal.hpp"
#include "cdpr_resample.hpp"

namespace cdpr_host {

// what both calls refuse of a request; P becomes the group size in robots
static int resample_checks(cdpr_engine* h, const cdpr_resample_spec_t* spec, const float* d_weights, uint32_t& P, const char* what) {
  const char* bad = nullptr;
  if (!spec) bad = "null spec";
  else if (spec->struct_size != sizeof(cdpr_resample_spec_t)) bad = "spec.struct_size is not sizeof(cdpr_resample_spec_t)";
  else if (spec->flags != 0u) bad = "spec.flags must be 0";
  else if (!(spec->ess_gate >= 0.0f)) bad = "spec.ess_gate is NaN or negative";
  else if (!d_weights) bad = "null weights";
  else if (h->batch % (spec->group_size ? spec->group_size : h->batch) != 0u) bad = "the batch is not a whole number of groups";
  if (bad) {
    h->err = std::string(what) + ": " + bad;
    return CDPR_ERR_INVALID;
  }
  P = spec->group_size ? spec->group_size : h->batch;
  if (P > kResampleMaxP) {
    h->err = std::string(what) + ": a group of more than 65 536 robots";
    return CDPR_ERR_UNSUPPORTED;
  }
  return CDPR_OK;
}

// Queue the map kernel behind everything queued so far, the five status words (or null) zeroed on the stream in front of it.
// fused: the copy kernel follows and counts the robots copied itself.
static int launch_resample_map(cdpr_engine* h, uint32_t P, float gate, const float* d_weights, const uint32_t* d_words, int32_t* d_source, float* d_ess,
                               uint32_t* d_status, bool fused) {
  if (int rc = zero_counts(h, d_status, 5)) return rc;
  ResampleArgs a{};
  a.weights = d_weights, a.words = d_words, a.source = d_source, a.ess = d_ess, a.status = d_status;
  a.group = P, a.groups = h->batch / P, a.gate = gate, a.count_destinations = fused ? 0u : 1u;
  const ResampleForm form = resample_form(P);
  if (form.lds > 64u * 1024u)  // (above the default limit of dynamic LDS a kernel asks for it by attribute)
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(form.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)form.lds));
  const dim3 grid((a.groups + form.groups_per_block - 1u) / form.groups_per_block), block(kResampleBlock);
  hipLaunchKernelGGL(form.kernel, grid, block, form.lds, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return CDPR_OK;
}

}  // namespace cdpr_host

extern "C" {

size_t cdpr_resample_spec_size(void) { return sizeof(cdpr_resample_spec_t); }

int cdpr_resample_map_device(cdpr_handle_t h, const cdpr_resample_spec_t* spec, const float* d_weights, const uint32_t* d_words, int32_t* d_source,
                             float* d_ess, uint32_t* d_status) {
  const char* const what = "cdpr_resample_map_device";
  if (!h) return CDPR_ERR_INVALID;
  uint32_t P = 0;
  if (int rc = resample_checks(h, spec, d_weights, P, what)) return rc;
  if (!d_source) {
    h->err = std::string(what) + ": null source map";
    return CDPR_ERR_INVALID;
  }
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_resample_map(h, P, spec->ess_gate, d_weights, d_words, d_source, d_ess, d_status, false);
}

int cdpr_resample_device(cdpr_handle_t h, const cdpr_resample_spec_t* spec, const float* d_weights, const uint32_t* d_words, int32_t* d_source,
                         float* d_ess, uint32_t* d_status) {
  const char* const what = "cdpr_resample_device";
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = per_robot_checks(h, what)) return rc;
  uint32_t P = 0;
  if (int rc = resample_checks(h, spec, d_weights, P, what)) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (!d_source) {  // the handle's own map (the scratch of cdpr_copy_robots' host form: stream order keeps the two apart)
    if (!h->d_copy_map) HIP_TRY(h, h->d_copy_map.alloc((size_t)h->batch * sizeof(int32_t)));
    d_source = h->d_copy_map;
  }
  if (int rc = launch_resample_map(h, P, spec->ess_gate, d_weights, d_words, d_source, d_ess, d_status, true)) return rc;
  return launch_copy(h, d_source, d_status, true);  // ([0] and [1]: the copy kernel's own counts, zeroed with the rest)
}

}  // extern "C"
