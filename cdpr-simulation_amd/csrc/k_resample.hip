// systematic resampling, weights to the source map of the fork (cdpr_resample.hpp): one kernel per form of group size
#include "cdpr_resample.hpp"
namespace cdpr {
ResampleForm resample_form(uint32_t P) {
  if (P <= kResampleWaveP) return {cdpr_resample_kernel<64u, 1u, true>, kResampleBlock / 64u, (kResampleBlock / 64u) * 64u * sizeof(uint16_t)};  // a wave per group
  const size_t lds = (((size_t)P + 1u) & ~(size_t)1u) * sizeof(uint16_t);
  if (P <= kResampleOneP) return {cdpr_resample_kernel<kResampleBlock, kResampleItems, true>, 1u, lds};  // a workgroup per group, weights in registers
  return {cdpr_resample_kernel<kResampleBlock, kResampleItems, false>, 1u, lds};                          // ... in chunks with carries
}
}  // namespace cdpr
