// general controller path in one launch per step (cdpr_general_step.hpp): stepping kernel, windows of 12 .. 32 samples
#include "cdpr_kernels.hpp"
#include "cdpr_general_step.hpp"
namespace cdpr {
namespace {
// cdpr_gen_step_kernel<N, FK, TD, ROLLOUT, NBMAX, SINGLE>
#define K_GEN(N, FK, TD) cdpr_gen_step_kernel<N, FK, TD, false, kGenMaxBuf, false>
template <int N> GenKernel gen_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_GEN); }
}  // namespace
GenKernel gen_step32_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  CDPR_PICK_CABLES(gen_n, k.fk, k.td);
}
}  // namespace cdpr
