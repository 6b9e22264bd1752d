// the environment view: observation tensor, reward and done verdict in one launch (cdpr_env.hpp), one kernel per platform layout
#include "cdpr_env.hpp"
namespace cdpr {
EnvKernel pick_env_kernel() { return cdpr_env_kernel<kEnvBlock>; }              // float4 slot rows: every fp32 handle
EnvF64Kernel pick_env_f64_kernel() { return cdpr_env_f64_kernel<kEnvBlock>; }  // double rows: precision = 64
}  // namespace cdpr
