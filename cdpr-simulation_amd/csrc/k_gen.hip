// cdpr_gen_step_kernel<N, FK, TD, ROLLOUT, NBMAX, SINGLE>: the one-wave general-path kernel is instantiated in five translation
// units (k_gen_one / _step / _roll / _step32 / _roll32.hip, one per (ROLLOUT, NBMAX, SINGLE) it exists in); this picks the unit
#include "cdpr_kernels.hpp"
namespace cdpr {
GenKernel gen_one11_entry(const PlannedKernel& k);
GenKernel gen_step11_entry(const PlannedKernel& k);
GenKernel gen_roll11_entry(const PlannedKernel& k);
GenKernel gen_step32_entry(const PlannedKernel& k);
GenKernel gen_roll32_entry(const PlannedKernel& k);
GenKernel gen_step_kernel_entry(const PlannedKernel& k) {
  if (k.rollout && k.single) return nullptr;
  if (k.nbmax == kGenMaxBuf) return k.rollout ? gen_roll32_entry(k) : k.single ? nullptr : gen_step32_entry(k);  // (long windows: no one-step build)
  if (k.nbmax != 11) return nullptr;
  if (k.rollout) return gen_roll11_entry(k);
  return k.single ? gen_one11_entry(k) : gen_step11_entry(k);
}
}  // namespace cdpr
