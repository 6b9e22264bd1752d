// cdpr_engine_copy.hip - cdpr_copy_robots / cdpr_copy_robots_device: robots of a per-robot handle continue from where other robots of
// the same handle are now, one launch of the copy kernel of the handle's record layout (take_over, cdpr_robot_records.hpp) on the
// handle's stream.  Neither form waits for the stream or copies anything back.  Not a step launch: h->last_kernel and the launch
// counter stay as they are.
#include "cdpr_engine_internal.hpp"

namespace cdpr {

// one thread per destination index; a non-destination leaves at once
template <typename View>
CDPR_DEV void copy_thread(const CopyWho& who, const View& v) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t s;
  if (copy_verdict(who, v.batch, r, s)) take_over(v, r, s);
}
static __global__ __launch_bounds__(256) void cdpr_copy_fast_kernel(const CopyWho who, const FastRecords v) { copy_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_copy_gen_kernel(const CopyWho who, const GenRecords v) { copy_thread(who, v); }
static __global__ __launch_bounds__(256) void cdpr_copy_f64_kernel(const CopyWho who, const F64Records v) { copy_thread(who, v); }

}  // namespace cdpr

namespace cdpr_host {

// Queue the copy behind every update queued so far.  d_source int32[B], d_status uint32[2] or null (zeroed on the stream first, unless
// the caller has done that: `zeroed`): device buffers.  The world step, the publish clock, the status word and every pending command
// stay as they are.  (Also the second launch of cdpr_resample_device, cdpr_engine_resample.hip.)
int launch_copy(cdpr_engine* h, const int32_t* d_source, uint32_t* d_status, bool zeroed) {
  if (!zeroed)
    if (int rc = zero_counts(h, d_status, 2)) return rc;
  return launch_per_robot(h, CopyWho{d_source, d_status}, cdpr_copy_fast_kernel, cdpr_copy_gen_kernel, cdpr_copy_f64_kernel, true);
}

}  // namespace cdpr_host

extern "C" {

int cdpr_copy_robots_device(cdpr_handle_t h, const int32_t* d_source, uint32_t* d_status) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = per_robot_checks(h, "cdpr_copy_robots_device", d_source ? nullptr : "source map")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return launch_copy(h, d_source, d_status);
}

int cdpr_copy_robots(cdpr_handle_t h, const int32_t* source) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = per_robot_checks(h, "cdpr_copy_robots", source ? nullptr : "source map")) return rc;
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
  // the map through the staging pair to the device scratch on the handle's stream
  const size_t bytes = B * sizeof(int32_t);
  if (!h->d_copy_map) HIP_TRY(h, h->d_copy_map.alloc(bytes));
  const auto fill = [&](char* stage) { memcpy(stage, source, bytes); };
  HIP_TRY(h, h->copy_stage.send(h->d_copy_map, bytes, h->stream, fill));
  return launch_copy(h, h->d_copy_map, nullptr);
}

}  // extern "C"
