// first-generation step kernel on uniform handles: one step, several steps, low-register, rollout, PHYS (see cdpr_kernels.hpp)
#include "cdpr_kernels.hpp"
namespace cdpr {
namespace {
// the family's positional template arguments, once:   <N, FK, TD, SINGLE, ROLLOUT, LOWREG, PHYS, PR>
#define K_STEP(N, FK, TD, SINGLE, ROLLOUT, LOWREG, PHYS) cdpr_step_kernel<N, FK, TD, SINGLE, ROLLOUT, LOWREG, PHYS, false>
// (the helpers below stand in the order the kernels have always been emitted in, which keeps the unit's code object comparable)
#define K_PLAIN(N, FK, TD) K_STEP(N, FK, TD, SINGLE, false, false, false)
template <int N, bool SINGLE> StepKernel stage(bool fk, bool td) { CDPR_PICK_STAGES(N, K_PLAIN); }
template <int N> StepKernel step_n(const PlannedKernel& k) { return k.single ? stage<N, true>(k.fk, k.td) : stage<N, false>(k.fk, k.td); }
#define K_ROLL(N, FK, TD) K_STEP(N, FK, TD, false, true, false, false)
template <int N> StepKernel roll_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_ROLL); }
// lumped-leg physics / joint stop (PHYS = true): one generic stepping kernel (any steps per launch) and the MPC rollout
#define K_PHYS_STEP(N, FK, TD) K_STEP(N, FK, TD, false, false, false, true)
#define K_PHYS_ROLL(N, FK, TD) K_STEP(N, FK, TD, false, true, false, true)
template <int N> StepKernel phys_step_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_PHYS_STEP); }
template <int N> StepKernel phys_roll_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_PHYS_ROLL); }
template <int N> StepKernel phys_n(const PlannedKernel& k) { return k.rollout ? phys_roll_n<N>(k.fk, k.td) : phys_step_n<N>(k.fk, k.td); }

// one step or several: to twelve cables
StepKernel plain(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES12(step_n, k);
}
StepKernel rollout(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES12(roll_n, k.fk, k.td);
}
StepKernel phys(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES(phys_n, k);
}
// one-step kernels compiled for two waves per SIMD (FK on, six to eight cables): see LOWREG in cdpr_step_kernel.hpp
StepKernel lowreg(const PlannedKernel& k) {
  switch (k.n) {
    case 6: return k.td ? K_STEP(6, true, true, true, false, true, false) : K_STEP(6, true, false, true, false, true, false);
    case 7: return k.td ? K_STEP(7, true, true, true, false, true, false) : K_STEP(7, true, false, true, false, true, false);
    case 8: return k.td ? K_STEP(8, true, true, true, false, true, false) : K_STEP(8, true, false, true, false, true, false);
  }
  return nullptr;
}
}  // namespace

StepKernel step_kernel_entry(const PlannedKernel& k) {
  if (k.per_robot) return nullptr;
  if (k.lowreg) return (k.fk && k.single && !k.rollout && !k.phys) ? lowreg(k) : nullptr;
  if (k.phys) return k.single ? nullptr : phys(k);
  if (k.rollout) return k.single ? nullptr : rollout(k);
  return plain(k);
}
}  // namespace cdpr
