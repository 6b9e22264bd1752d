// MPPI: the sampler of the command batch and the update of the plan, one instantiation per cable count (cdpr_mppi.hpp)
#include "cdpr_mppi.hpp"
#include "cdpr_kernels.hpp"
namespace cdpr {
template <int N>
static MppiUpdateKernel update_n(uint32_t) { return cdpr_mppi_update_kernel<N>; }
MppiUpdateKernel mppi_update_kernel_entry(uint32_t n) { CDPR_PICK_CABLES12(update_n, n); }
MppiSampleKernel mppi_sample_kernel_entry(bool vec) { return vec ? cdpr_mppi_sample_kernel<true> : cdpr_mppi_sample_kernel<false>; }
}  // namespace cdpr
