// two lanes per robot (cdpr_step_kernel_pair.hpp), n = 4 or 8
#include "cdpr_kernels.hpp"
#include "cdpr_step_kernel_pair.hpp"
namespace cdpr {
namespace {
// cdpr_step_kernel_pair<N, FK, TD, SINGLE>
#define K_PAIR(N, FK, TD) cdpr_step_kernel_pair<N, FK, TD, SINGLE>
template <int N, bool SINGLE> StepKernel stage(bool fk, bool td) { CDPR_PICK_STAGES(N, K_PAIR); }
template <int N> StepKernel pair_n(const PlannedKernel& k) { return k.single ? stage<N, true>(k.fk, k.td) : stage<N, false>(k.fk, k.td); }
// cdpr_pair_stream_kernel<N, VEL>: the steady-state several-steps launch of FK-less, TD-less handles; VEL: the Pid sees the joint velocity
template <int N> StepKernel stream_n(const PlannedKernel& k) { return k.vel ? cdpr_pair_stream_kernel<N, true> : cdpr_pair_stream_kernel<N, false>; }
}  // namespace
StepKernel pair_kernel_entry(const PlannedKernel& k) {
  if (k.n == 4) return pair_n<4>(k);
  if (k.n == 8) return pair_n<8>(k);
  return nullptr;
}
StepKernel pair_stream_kernel_entry(const PlannedKernel& k) {
  if (k.fk || k.td || k.single) return nullptr;
  if (k.n == 4) return stream_n<4>(k);
  if (k.n == 8) return stream_n<8>(k);
  return nullptr;
}
}  // namespace cdpr
