// precision = 64: the step in the reference's own precision (cdpr_step_kernel_f64.hpp)
#include "cdpr_kernels.hpp"
namespace cdpr {
// the one-wave kernel's other units: TSTOP (k_f64_phys.hip), W = 31 (k_f64_long.hip), HW = 32 (k_f64_hold_long.hip)
F64Kernel f64_phys_entry(const PlannedKernel& k);
F64Kernel f64_long_entry(const PlannedKernel& k);
F64Kernel f64_hold_long_entry(const PlannedKernel& k);
namespace {
// the family's positional template arguments, once:   <N, RING_LDS, JCACHE, PR, HOLD, TSTOP, W, HW>
#define K_F64(N, RING_LDS, JCACHE, PR, HOLD) cdpr_step_kernel_f64<N, RING_LDS, JCACHE, PR, HOLD, false, kWin, kHoldWin>
// (the helpers below stand in the order the kernels have always been emitted in, which keeps the unit's code object comparable)
// per-robot handles (mode, call count and Pid per lane); ring_lds: the derivative rings staged in LDS (small batches)
template <int N> F64Kernel f64_pr_n(bool ring_lds) { return ring_lds ? K_F64(N, true, false, true, 0) : K_F64(N, false, false, true, 0); }
// ... and on uniform handles; jcache: the structure-matrix rows in LDS too (112 KiB of LDS per wave at n = 8: one workgroup per CU)
template <int N> F64Kernel f64_n(bool ring_lds, bool jcache) {
  if (jcache) return ring_lds ? K_F64(N, true, true, false, 0) : nullptr;
  return ring_lds ? K_F64(N, true, false, false, 0) : K_F64(N, false, false, false, 0);
}
// HOLD: velocityEpsilon >= 0, the position-hold branch live (both Pids of every cable); 2: + biquad cascades, cmd_limit 0
template <int N> F64Kernel f64_hold_n(int hold) { return hold == 2 ? K_F64(N, false, false, false, 2) : K_F64(N, false, false, false, 1); }
template <int N> F64Kernel f64_hold_pr_n(int hold) { return hold == 2 ? K_F64(N, false, false, true, 2) : K_F64(N, false, false, true, 1); }
F64Kernel hold_pr(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES(f64_hold_pr_n, k.hold);
}
F64Kernel hold(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES(f64_hold_n, k.hold);
}
// nine to twelve cables: the plain one-wave kernel, rings in memory (the LDS variants' columns do not fit)
template <int N> F64Kernel f64_n12(bool ring_lds, bool jcache) {
  if constexpr (N > 8)
    return (ring_lds || jcache) ? nullptr : K_F64(N, false, false, false, 0);
  else
    return f64_n<N>(ring_lds, jcache);
}
F64Kernel plain(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES12(f64_n12, k.f64_ring_lds, k.f64_jcache);
}
F64Kernel pr(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES(f64_pr_n, k.f64_ring_lds);
}
// cdpr_split_kernel_f64<N, LEAN, HOLD>: one step per launch, two waves per 64 robots split by role (FK + TD, six to eight cables);
// LEAN: nothing cached in LDS (four workgroups per CU)
template <int HOLD> F64Kernel f64_split(uint32_t n, bool lean) {
  if (lean) {
    switch (n) {
      case 6: return cdpr_split_kernel_f64<6, true, HOLD>;
      case 7: return cdpr_split_kernel_f64<7, true, HOLD>;
      case 8: return cdpr_split_kernel_f64<8, true, HOLD>;
    }
    return nullptr;
  }
  switch (n) {
    case 6: return cdpr_split_kernel_f64<6, false, HOLD>;
    case 7: return cdpr_split_kernel_f64<7, false, HOLD>;
    case 8: return cdpr_split_kernel_f64<8, false, HOLD>;
  }
  return nullptr;
}
}  // namespace
F64Kernel f64_step_kernel_entry(const PlannedKernel& k) {
  if (k.hold_w32) return f64_hold_long_entry(k);
  if (k.win31) return f64_long_entry(k);
  if (k.tstop) return f64_phys_entry(k);
  if (k.hold) return (k.f64_ring_lds || k.f64_jcache) ? nullptr : k.per_robot ? hold_pr(k) : hold(k);
  if (k.per_robot) return k.f64_jcache ? nullptr : pr(k);
  return plain(k);
}
F64Kernel f64_split_kernel_entry(const PlannedKernel& k) {
  if (k.per_robot) return nullptr;
  return k.hold == 2 ? f64_split<2>(k.n, k.f64_lean) : k.hold == 1 ? f64_split<1>(k.n, k.f64_lean) : f64_split<0>(k.n, k.f64_lean);
}
}  // namespace cdpr
