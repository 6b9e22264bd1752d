// second-generation one-step kernel (controller rows staged through LDS) and the role-split kernel, uniform and PR
#include "cdpr_kernels.hpp"
#include "cdpr_onestep_kernel.hpp"
namespace cdpr {
namespace {
// cdpr_onestep_kernel<N, FK, TD, PERSIST>; PERSIST: one wave per SIMD walking over blocks of 64 robots
#define K_ONE(N, FK, TD) cdpr_onestep_kernel<N, FK, TD, false>
#define K_ONE_PERSIST(N, FK, TD) cdpr_onestep_kernel<N, FK, TD, true>
template <int N> StepKernel one_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_ONE); }
template <int N> StepKernel one_persist_n(bool fk, bool td) { CDPR_PICK_STAGES(N, K_ONE_PERSIST); }
}  // namespace
StepKernel onestep_kernel_entry(const PlannedKernel& k) {
  const uint32_t n = k.n;
  if (!k.single || k.per_robot) return nullptr;
  if (!k.persist) {
    CDPR_PICK_CABLES(one_n, k.fk, k.td);
  }
  CDPR_PICK_CABLES(one_persist_n, k.fk, k.td);
}
// The role-split kernels, six to eight cables (FK + TD handles): cdpr_split_kernel<N, PR> and, for a uniform handle's steady-state
// launches, the same kernel with both waves' steady-state instantiations, cdpr_split_steady_kernel<N, VEL>
#define CDPR_PICK_SPLIT(K)  \
  switch (k.n) {            \
    case 6: return K(6);    \
    case 7: return K(7);    \
    case 8: return K(8);    \
  }                         \
  return nullptr
#define K_SPLIT(N) cdpr_split_kernel<N, false>
#define K_SPLIT_STEADY(N) (k.vel ? cdpr_split_steady_kernel<N, true> : cdpr_split_steady_kernel<N, false>)
#define K_SPLIT_PR(N) cdpr_split_kernel<N, true>
StepKernel split_kernel_entry(const PlannedKernel& k) {
  if (!k.per_robot && !k.steady) {
    CDPR_PICK_SPLIT(K_SPLIT);
  }
  if (!k.per_robot) {
    CDPR_PICK_SPLIT(K_SPLIT_STEADY);
  }
  if (k.steady) return nullptr;
  CDPR_PICK_SPLIT(K_SPLIT_PR);
}
}  // namespace cdpr
