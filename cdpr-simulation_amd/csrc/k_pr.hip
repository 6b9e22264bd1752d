// per-robot handles on the register-resident path (PR = true): the first-generation kernel in every shape (one step,
// several steps, low-register, rollout); the role-split PR kernel lives in k_onestep.hip
#include "cdpr_kernels.hpp"
namespace cdpr {
namespace {
// the family's positional template arguments, once:   <N, FK, TD, SINGLE, ROLLOUT, LOWREG, PHYS, PR>
#define K_PR(N, FK, TD, SINGLE, ROLLOUT, LOWREG) cdpr_step_kernel<N, FK, TD, SINGLE, ROLLOUT, LOWREG, false, true>
template <int N, bool SINGLE, bool ROLLOUT, bool LOWREG>
StepKernel stage(bool fk, bool td) {
  if constexpr (N >= 6) {
    if (fk && td) return K_PR(N, true, true, SINGLE, ROLLOUT, LOWREG);
    if (fk) return K_PR(N, true, false, SINGLE, ROLLOUT, LOWREG);
    if constexpr (!LOWREG)
      if (td) return K_PR(N, false, true, SINGLE, ROLLOUT, false);
  }
  if constexpr (!LOWREG) return K_PR(N, false, false, SINGLE, ROLLOUT, false);
  return nullptr;  // (the low-register build exists with FK on, from six cables)
}
template <int N>
StepKernel pr_n(const PlannedKernel& k) {
  if (k.rollout) return (k.single || k.lowreg) ? nullptr : stage<N, false, true, false>(k.fk, k.td);
  if (!k.single) return k.lowreg ? nullptr : stage<N, false, false, false>(k.fk, k.td);
  return k.lowreg ? stage<N, true, false, true>(k.fk, k.td) : stage<N, true, false, false>(k.fk, k.td);
}
}  // namespace
StepKernel pr_step_kernel_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  if (!k.per_robot || k.phys) return nullptr;
  CDPR_PICK_CABLES(pr_n, k);
}
}  // namespace cdpr
