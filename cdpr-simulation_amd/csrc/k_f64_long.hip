// precision = 64 with derivative windows of 12 .. 32 samples (W = kWinLong: a ring of 31 errors per cable on the one-wave kernel) - alone
// and together with per-robot modes and / or the optional physics
#include "cdpr_kernels.hpp"
namespace cdpr {
namespace {
// cdpr_step_kernel_f64<N, RING_LDS, JCACHE, PR, HOLD, TSTOP, W, HW>
template <int N, bool PR, bool TSTOP> F64Kernel f64_long_n() { return cdpr_step_kernel_f64<N, false, false, PR, 0, TSTOP, kWinLong>; }
template <int N> F64Kernel f64_long_any(bool pr, bool tstop) {
  if (pr) return tstop ? f64_long_n<N, true, true>() : f64_long_n<N, true, false>();
  return tstop ? f64_long_n<N, false, true>() : f64_long_n<N, false, false>();
}
}  // namespace
F64Kernel f64_long_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  if (!k.win31 || k.f64_ring_lds || k.f64_jcache || k.hold || k.hold_w32) return nullptr;
  CDPR_PICK_CABLES(f64_long_any, k.per_robot, k.tstop);
}
}  // namespace cdpr
