// precision = 64: the hold branch / cascades / cmd_limit 0 with derivative windows of 12 .. 32 samples: the HOLD = 2 instantiations of
// the one-wave kernel over Pid records of 32 samples (HW = kHoldWinLong) - uniform and per-robot handles, with and without the
// optional physics
#include "cdpr_kernels.hpp"
namespace cdpr {
namespace {
// cdpr_step_kernel_f64<N, RING_LDS, JCACHE, PR, HOLD, TSTOP, W, HW>
template <int N, bool PR, bool TSTOP> F64Kernel f64_hold_long_n() { return cdpr_step_kernel_f64<N, false, false, PR, 2, TSTOP, kWin, kHoldWinLong>; }
template <int N> F64Kernel f64_hold_long_any(bool pr, bool tstop) {
  if (pr) return tstop ? f64_hold_long_n<N, true, true>() : f64_hold_long_n<N, true, false>();
  return tstop ? f64_hold_long_n<N, false, true>() : f64_hold_long_n<N, false, false>();
}
}  // namespace
F64Kernel f64_hold_long_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  if (!k.hold_w32 || k.hold != 2 || k.f64_ring_lds || k.f64_jcache || k.win31) return nullptr;
  CDPR_PICK_CABLES(f64_hold_long_any, k.per_robot, k.tstop);
}
}  // namespace cdpr
