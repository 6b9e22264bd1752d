// cdpr_engine_reset.hip - cdpr_reset_robots / cdpr_reset_robots_device: the model reset of chosen robots of a per-robot handle, one
// launch of the reset kernel of the handle's record layout (model_reset, cdpr_robot_records.hpp) on the handle's stream.  Neither
// form waits for the stream or copies anything back.  Reference paths as in cdpr_engine.hip.
#include "cdpr_engine_internal.hpp"

namespace cdpr {

template <typename View>
CDPR_DEV void reset_thread(const ResetWhere& who, const View& v) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < v.batch && who.mask[r]) model_reset(who, v, r);  // (a robot outside the mask: its pose and twist rows are never read)
}
static __global__ __launch_bounds__(256) void cdpr_reset_fast_kernel(const ResetWhere who, const FastRecords v) { reset_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_reset_gen_kernel(const ResetWhere who, const GenRecords v) { reset_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_reset_f64_kernel(const ResetWhere who, const F64Records v) { reset_thread(who, v); }

}  // namespace cdpr

namespace cdpr_host {

// Queue the reset behind every update queued so far.  d_mask uint8[B], d_pose float[B][7] or null (home), d_twist float[B][6] or null
// (zero): device buffers.  h->mode, h->pid_calls (not used on per-robot handles), the world step, the publish clock, the status word
// and every pending command stay as they are; the reset robots' episode clock takes the world step of the call.  (Also the second
// launch of cdpr_reset_done_device, cdpr_engine_done.hip.)
int launch_reset(cdpr_engine* h, const uint8_t* d_mask, const float* d_pose, const float* d_twist) {
  ResetWhere who{};
  who.mask = d_mask, who.pose = d_pose, who.twist = d_twist, who.step = (uint32_t)h->step;
  for (int c = 0; c < 7; ++c) who.home[c] = (float)h->cfg.home_pose[c];
  return launch_per_robot(h, who, cdpr_reset_fast_kernel, cdpr_reset_gen_kernel, cdpr_reset_f64_kernel, true);
}

}  // namespace cdpr_host

extern "C" {

int cdpr_reset_robots_device(cdpr_handle_t h, const uint8_t* d_robot_mask, const float* d_pose7, const float* d_twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = per_robot_checks(h, "cdpr_reset_robots_device", d_robot_mask ? nullptr : "robot mask")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_reset(h, d_robot_mask, d_pose7, d_twist6);
}

int cdpr_reset_robots(cdpr_handle_t h, const uint8_t* robot_mask, const float* pose7, const float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = per_robot_checks(h, "cdpr_reset_robots", robot_mask ? nullptr : "robot mask")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  // [mask, padded to 16 B | pose | twist] through the staging pair to the device scratch on the handle's stream
  const size_t B = h->batch, off_pose = (B + 15u) & ~(size_t)15u, off_twist = off_pose + B * 7 * sizeof(float), bytes = off_twist + B * 6 * sizeof(float);
  if (!h->d_reset_args) HIP_TRY(h, h->d_reset_args.alloc(bytes));
  const auto fill = [&](char* stage) {
    memcpy(stage, robot_mask, B);
    if (pose7) memcpy(stage + off_pose, pose7, B * 7 * sizeof(float));
    if (twist6) memcpy(stage + off_twist, twist6, B * 6 * sizeof(float));
  };
  HIP_TRY(h, h->reset_stage.send(h->d_reset_args, bytes, h->stream, fill));
  char* const d = h->d_reset_args;
  return launch_reset(h, reinterpret_cast<const uint8_t*>(d), pose7 ? reinterpret_cast<const float*>(d + off_pose) : nullptr,
                      twist6 ? reinterpret_cast<const float*>(d + off_twist) : nullptr);
}

}  // extern "C"
