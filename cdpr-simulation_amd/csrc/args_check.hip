// args_check.hip - the argument builders as a stand-alone host program (`make args-check`: built under the address and undefined-behaviour
// sanitizers, needs no device): launch_args and launch_args_image (cdpr_launch_args.hpp) over dispatch_check.hip's configuration matrix -
// cable counts 1 .. 12, the six handle kinds with and without per-robot commands, both precisions, every mode - and over the widest
// shapes the arrays allow: windows of 32 samples, four cascade stages on every filter, cmd_limit = 0, i_gain = 0.  Two builds of a cell
// must be the same bytes, also when the memory they are built in held something else before (padding is zeroed, nothing is read
// uninitialised); a sanitizer report ends the program with a non-zero status.
#include <cstring>
#include <new>

#include "cdpr_launch_args.hpp"

using namespace cdpr_host;

static cdpr_config_t base_config(uint32_t n, uint64_t batch, uint32_t stages) {  // (dispatch_check.hip's)
  cdpr_config_t c;
  memset(&c, 0, sizeof c);
  c.abi_version = CDPR_ABI_VERSION;
  c.n_cables = n, c.batch = batch, c.dt = 1e-3, c.mass = 1.0, c.stages = stages;
  c.inertia[0] = c.inertia[1] = c.inertia[2] = 0.1;
  for (uint32_t i = 0; i < n; ++i) c.cable_ref_length[i] = 1.0;
  for (cdpr_pid_params_t* p : {&c.velocity_pid, &c.position_pid}) p->d_degree = 2, p->d_buffer_length = 11, p->cmd_limit = 100.0, p->i_limit = 1.0, p->i_gain = 2.0;
  c.velocity_epsilon = -1.0;
  c.fk_max_iterations = 4, c.td_f_min = 5.0, c.td_f_max = 100.0;
  return c;
}

// the image of one cell, built in storage filled with `fill` first: a byte the builders leave unwritten shows as a difference
static std::vector<unsigned char> image_over(const cdpr_config_t& c, const KernelPlan& plan, int mode, int fill) {
  alignas(LaunchArgs) static unsigned char storage[sizeof(LaunchArgs)];
  memset(storage, fill, sizeof storage);
  LaunchArgs* L = new (storage) LaunchArgs(launch_args(c, plan, no_env));
  std::vector<unsigned char> image = launch_args_image(*L, plan, mode);
  L->~LaunchArgs();
  return image;
}

int main() {
  long cells = 0, refused = 0, bad = 0;
  for (uint32_t n = 1; n <= CDPR_MAX_CABLES; ++n)
    for (int kind = 0; kind < 16; ++kind)
      for (uint32_t precision : {32u, 64u}) {
        cdpr_config_t c = base_config(n, 65, n >= 6 ? (uint32_t)(CDPR_STAGE_FK | CDPR_STAGE_TD) : 0u);
        c.per_robot_commands = (kind & 1) != 0;
        c.precision = precision;
        switch (kind >> 1) {
          case 0: break;                                                   // register-resident
          case 1: c.velocity_epsilon = 0.001; break;                       // the hold branch
          case 2: c.velocity_pid.d_buffer_length = c.position_pid.d_buffer_length = 21; break;  // long windows
          case 3: c.velocity_epsilon = 0.001, c.velocity_pid.d_buffer_length = 21; break;       // both
          case 4: c.travel_lower = -0.01, c.travel_upper = 0.01, c.travel_stop = 2, c.leg_inertia = 0.004; break;  // optional physics
          case 5: c.velocity_pid.p_filter.cascade = 1, c.velocity_pid.p_filter.rel_cutoff = 0.1, c.velocity_pid.p_filter.quality = 0.7, c.leg_inertia = 0.004; break;
          case 6:  // the widest shapes: every window 32 samples of degree 4, every filter four stages deep, no command clamp, no integral
          case 7:  // ... with the hold branch live
            for (cdpr_pid_params_t* p : {&c.velocity_pid, &c.position_pid}) {
              p->d_buffer_length = CDPR_MAX_D_BUFFER, p->d_degree = CDPR_MAX_D_DEGREE, p->cmd_limit = 0.0, p->i_gain = 0.0, p->i_limit = -3.0;
              for (cdpr_filter_params_t* f : {&p->p_filter, &p->d_filter}) f->cascade = CDPR_MAX_CASCADE, f->rel_cutoff = 0.2, f->quality = 0.6;
            }
            if ((kind >> 1) == 7) c.velocity_epsilon = 0.004;
            break;
        }
        const KernelPlan plan = plan_kernels(c, 256, no_env);
        if (plan.rc != CDPR_OK) {
          ++refused;
          continue;
        }
        for (int mode = kModeForce; mode <= kModeVelocity; ++mode) {
          ++cells;
          const std::vector<unsigned char> a = image_over(c, plan, mode, 0x00), b = image_over(c, plan, mode, 0xa5);
          const size_t record = plan.fp64 ? sizeof(F64Args) : plan.general ? sizeof(StepArgs) + sizeof(GenCtl) : sizeof(StepArgs);
          if (a.size() <= record || a.size() != b.size() || memcmp(a.data(), b.data(), a.size()) != 0)
            ++bad, printf("two builds differ: n %u kind %d precision %u mode %d\n", n, kind, precision, mode);
        }
        // the Pid record itself, and the rules it states once
        const PidTerms t = pid_terms(c.velocity_pid);
        if (t.imax < 0.0 || t.imin != -t.imax || t.cmin != -t.cmax || t.clamp != (c.velocity_pid.cmd_limit != 0.0) || (c.velocity_pid.i_gain == 0.0) != (t.inv_ki == 0.0))
          ++bad, printf("pid_terms breaks a rule: n %u kind %d\n", n, kind);
      }
  printf("args_check: %ld cells (%ld configurations refused), %ld failures\n", cells, refused, bad);
  return (bad || cells < 500) ? 1 : 0;
}
