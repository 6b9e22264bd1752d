// CEM: the update of the mean and sigma plans, one instantiation per cable count, and the sampler with sigma from a plan (cdpr_cem.hpp)
#include "cdpr_cem.hpp"
#include "cdpr_kernels.hpp"
namespace cdpr {
template <int N>
static CemUpdateKernel update_n(uint32_t) { return cdpr_cem_update_kernel<N>; }
CemUpdateKernel cem_update_kernel_entry(uint32_t n) { CDPR_PICK_CABLES12(update_n, n); }
MppiSampleKernel cem_sample_kernel_entry(bool vec) { return vec ? cdpr_mppi_sample_kernel<true, true> : cdpr_mppi_sample_kernel<false, true>; }
}  // namespace cdpr
