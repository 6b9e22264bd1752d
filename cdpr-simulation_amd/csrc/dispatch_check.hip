// dispatch_check.hip - the dispatch as a stand-alone host program (`make dispatch-check`: built under the address and undefined-behaviour
// sanitizers, needs no device): plan_kernels, planned_kernel, planned_kernel_name and the entry lookups over a matrix wider than the
// table test's - cable counts, stages, batches around every routing threshold, handle kinds (uniform, per-robot, general with short and
// long windows, precision = 64 with the hold branch, long windows, the optional physics), mappings, the routing overrides of the
// environment, every launch form and the precision = 64 per-call overrides.  Every planned kernel must have an instantiation, in both
// modes and in its steady form, and a name and an entry point must stand for each other.
#include <cstring>
#include <map>

#include "cdpr_kernels.hpp"

using namespace cdpr;

static std::map<std::string, std::string> g_env;
static const char* table_env(const char* key) {
  auto it = g_env.find(key);
  return it == g_env.end() ? nullptr : it->second.c_str();
}

static cdpr_config_t base_config(uint32_t n, uint64_t batch, uint32_t stages) {
  cdpr_config_t c;
  memset(&c, 0, sizeof c);
  c.abi_version = CDPR_ABI_VERSION;
  c.n_cables = n, c.batch = batch, c.dt = 1e-3, c.mass = 1.0, c.stages = stages;
  c.inertia[0] = c.inertia[1] = c.inertia[2] = 0.1;
  for (uint32_t i = 0; i < n; ++i) c.cable_ref_length[i] = 1.0;
  for (cdpr_pid_params_t* p : {&c.velocity_pid, &c.position_pid}) p->d_degree = 2, p->d_buffer_length = 11, p->cmd_limit = 100.0, p->i_limit = 1.0;
  c.velocity_epsilon = -1.0;
  c.fk_max_iterations = 4, c.td_f_min = 5.0, c.td_f_max = 100.0;
  return c;
}

int main() {
  std::map<std::string, const void*> entry_of_name;
  std::map<const void*, std::string> name_of_entry;
  long configs = 0, refused = 0, kernels = 0, bad = 0;
  const char* overrides[][2] = {{nullptr, nullptr},      {"CDPR_MAPPING", "1"},   {"CDPR_MAPPING", "2"},   {"CDPR_MAPPING", "3"},  {"CDPR_LOWREG", "1"},   {"CDPR_LOWREG", "0"},
                                {"CDPR_PERSIST", "1"},   {"CDPR_ONESTEP", "1"},   {"CDPR_SPLIT", "0"},     {"CDPR_CHUNK", "64"},   {"CDPR_PAIR_STREAM", "0"},
                                {"CDPR_GEN_SPLIT", "0"}, {"CDPR_GEN_SPLIT", "1"}, {"CDPR_GEN_LEAN", "1"},  {"CDPR_GEN_HOT", "0"}};
  for (const auto& ov : overrides) {
    g_env.clear();
    if (ov[0]) g_env[ov[0]] = ov[1];
    for (uint32_t n = 1; n <= CDPR_MAX_CABLES; ++n)
      for (uint32_t stages : {0u, (uint32_t)CDPR_STAGE_FK, (uint32_t)CDPR_STAGE_TD, (uint32_t)(CDPR_STAGE_FK | CDPR_STAGE_TD)})
        for (uint64_t batch : {1ull, 65ull, 4096ull, 16384ull, 16385ull, 32768ull, 32769ull, 65536ull, 65537ull, 90112ull, 90113ull, 131072ull, 524288ull})
          for (int kind = 0; kind < 12; ++kind)
            for (uint32_t mapping = 0; mapping <= (ov[0] ? 0u : (uint32_t)CDPR_MAP_LANE_PER_CABLE); ++mapping) {
              cdpr_config_t c = base_config(n, batch, stages);
              c.mapping = mapping;
              c.per_robot_commands = (kind & 1) != 0;
              switch (kind >> 1) {
                case 0: break;                                                   // register-resident
                case 1: c.velocity_epsilon = 0.001; break;                       // the hold branch
                case 2: c.velocity_pid.d_buffer_length = c.position_pid.d_buffer_length = 21; break;  // long windows
                case 3: c.velocity_epsilon = 0.001, c.velocity_pid.d_buffer_length = 21; break;       // both
                case 4: c.travel_lower = -0.01, c.travel_upper = 0.01, c.travel_stop = 2, c.leg_inertia = 0.004; break;  // optional physics
                case 5: c.velocity_pid.p_filter.cascade = 1, c.velocity_pid.p_filter.rel_cutoff = 0.1, c.velocity_pid.p_filter.quality = 0.7, c.leg_inertia = 0.004; break;
              }
              for (uint32_t precision : {32u, 64u}) {
                c.precision = precision;
                const KernelPlan plan = plan_kernels(c, 256, table_env);
                ++configs;
                if (plan.rc != CDPR_OK) {
                  ++refused;
                  if (plan.error.empty()) ++bad, printf("refused without a reason: n %u kind %d\n", n, kind);
                  continue;
                }
                for (int steps : {1, 10})
                  for (int form = 0; form < 16; ++form)
                    for (int f64_override = -1; f64_override <= (plan.fp64 ? 2 : -1); ++f64_override) {
                      LaunchShape s;
                      s.steps = steps;
                      s.first_world = form & 1, s.scheduled = (form & 2) != 0, s.rollout = (form & 4) != 0, s.steady = (form & 8) != 0;
                      s.f64_split = f64_override, s.f64_ring_lds = s.f64_jcache = f64_override < 0 ? -1 : (f64_override & 1);
                      const PlannedKernel missing = missing_entry(plan, s);
                      if (missing.id != KernelId::None) ++bad, printf("no instantiation for %s\n", planned_kernel_name(missing).c_str());
                      for (int variant = 0; variant < 4; ++variant) {
                        s.vel = variant & 1, s.split_steady = (variant & 2) != 0;
                        const PlannedKernel k = planned_kernel(plan, s);
                        const void* entry = entry_address(k);
                        std::string name = planned_kernel_name(k);
                        if (name.empty() || !entry || k.block == 0 || k.robots_per_block == 0 || k.grid(batch) == 0) { ++bad; continue; }
                        ++kernels;
                        // what the name leaves out on purpose (planned_kernel_name): the steady form and VEL, hot rows (a launch argument),
                        // and the one-step launch over long windows, which runs the several-steps instantiation
                        name = name.substr(0, name.find(" + hot rows")) + (k.steady ? " steady" : "") + (k.vel ? " VEL" : "");
                        if (k.id == KernelId::GenOne && k.nbmax != 11) continue;
                        auto a = entry_of_name.emplace(name, entry);
                        auto b = name_of_entry.emplace(entry, name);
                        if (a.first->second != entry || b.first->second != name) ++bad, printf("%s and %s share a name or an entry\n", name.c_str(), b.first->second.c_str());
                      }
                    }
              }
            }
  }
  printf("dispatch_check: %ld configurations (%ld refused), %ld planned kernels, %zu instantiations reached, %ld failures\n", configs, refused, kernels,
         entry_of_name.size(), bad);
  return bad ? 1 : 0;
}
