// general controller path, one step per launch, role-split form (cdpr_general_split.hpp): FK + TD handles, six to eight cables, windows up to 11 samples
#include "cdpr_kernels.hpp"
#include "cdpr_general_split.hpp"
namespace cdpr {
// cdpr_gen_split_kernel<N, NBMAX>: two waves per 64 robots split by role
GenKernel gen_split_kernel_entry(const PlannedKernel& k) {
  if (k.nbmax != 11) return nullptr;
  switch (k.n) {
    case 6: return cdpr_gen_split_kernel<6, 11>;
    case 7: return cdpr_gen_split_kernel<7, 11>;
    case 8: return cdpr_gen_split_kernel<8, 11>;
  }
  return nullptr;
}
// cdpr_gen_lean_kernel<N>: the same for larger batches: two waves per SIMD, the rare controller paths by call
GenKernel gen_lean_kernel_entry(const PlannedKernel& k) {
  if (k.nbmax != 11) return nullptr;
  switch (k.n) {
    case 6: return cdpr_gen_lean_kernel<6>;
    case 7: return cdpr_gen_lean_kernel<7>;
    case 8: return cdpr_gen_lean_kernel<8>;
  }
  return nullptr;
}
}  // namespace cdpr
