// precision = 64 with the optional physics (joint stop, lumped legs: the TSTOP instantiations of cdpr_step_kernel_f64) - alone, and
// together with per-robot modes and / or the hold branch: the world step does not care who set the forces
#include "cdpr_kernels.hpp"
namespace cdpr {
namespace {
// cdpr_step_kernel_f64<N, RING_LDS, JCACHE, PR, HOLD, TSTOP, W, HW>
template <int N, bool PR, int HOLD> F64Kernel f64_tstop_n() { return cdpr_step_kernel_f64<N, false, false, PR, HOLD, true>; }
template <int N> F64Kernel f64_tstop_any(bool pr, int hold) {
  if (pr) return hold == 2 ? f64_tstop_n<N, true, 2>() : hold == 1 ? f64_tstop_n<N, true, 1>() : f64_tstop_n<N, true, 0>();
  return hold == 2 ? f64_tstop_n<N, false, 2>() : hold == 1 ? f64_tstop_n<N, false, 1>() : f64_tstop_n<N, false, 0>();
}
}  // namespace
F64Kernel f64_phys_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  if (!k.tstop || k.f64_ring_lds || k.f64_jcache || k.win31 || k.hold_w32) return nullptr;
  CDPR_PICK_CABLES(f64_tstop_any, k.per_robot, k.hold);
}
}  // namespace cdpr
