// cdpr_kernels.hpp — from a kernel descriptor to its entry point.  planned_kernel (cdpr_select.hpp) names one instantiation
// completely in a PlannedKernel; the three lookups below, one per argument type, switch on its id once and hand it to the
// translation unit that instantiates the family (k_*.hip: one unit per family, they compile in parallel).  A unit's lookup reads the
// descriptor's fields and returns nullptr where it holds no such instantiation; the host refuses such a handle or call (refuse_missing).
//
// Adding a variant takes three places and no other:
//   1. a field of PlannedKernel for the new template argument, set in planned_kernel (cdpr_select.hpp);
//   2. the instantiation in the family's unit, behind the unit's lookup - the positional template arguments stand once per family
//      there, beside the names of the kernel's template parameters;
//   3. the label in planned_kernel_name (cdpr_select.hpp).
// A new family also takes a KernelId, its line in the lookup of its argument type below and a unit of its own (csrc/Makefile).
// Launch sites read planned_kernel -> entry -> launch, with the grid and block from the descriptor.
#pragma once
#include "cdpr_select.hpp"
#include "cdpr_step_kernel.hpp"
#include "cdpr_step_kernel_f64.hpp"
#include "cdpr_general_step.hpp"

namespace cdpr {

using StepKernel = void (*)(const StepArgs);
using F64Kernel = void (*)(const F64Args);
using GenKernel = void (*)(const StepArgs, const GenCtl);

// FK / TD exist from six cables on: below that the stage flags fall back to the plain instantiation
#define CDPR_PICK_STAGES(N, EXPR)                 \
  do {                                            \
    if constexpr ((N) >= 6) {                     \
      if (fk && td) return EXPR(N, true, true);   \
      if (fk) return EXPR(N, true, false);        \
      if (td) return EXPR(N, false, true);        \
    }                                             \
    return EXPR(N, false, false);                 \
  } while (0)
#define CDPR_PICK_CABLES(FN, ...)          \
  switch (n) {                             \
    case 1: return FN<1>(__VA_ARGS__);     \
    case 2: return FN<2>(__VA_ARGS__);     \
    case 3: return FN<3>(__VA_ARGS__);     \
    case 4: return FN<4>(__VA_ARGS__);     \
    case 5: return FN<5>(__VA_ARGS__);     \
    case 6: return FN<6>(__VA_ARGS__);     \
    case 7: return FN<7>(__VA_ARGS__);     \
    case 8: return FN<8>(__VA_ARGS__);     \
  }                                        \
  return nullptr

// nine to twelve cables (cube.yaml's `points` list is free-length): the first-generation kernel and the MPC rollout only
#define CDPR_PICK_CABLES12(FN, ...)        \
  switch (n) {                             \
    case 9: return FN<9>(__VA_ARGS__);     \
    case 10: return FN<10>(__VA_ARGS__);   \
    case 11: return FN<11>(__VA_ARGS__);   \
    case 12: return FN<12>(__VA_ARGS__);   \
  }                                        \
  CDPR_PICK_CABLES(FN, __VA_ARGS__)

// One lookup per kernel family, exported by the unit that instantiates it
StepKernel step_kernel_entry(const PlannedKernel& k);          // k_step.hip: cdpr_step_kernel, uniform handles
StepKernel pr_step_kernel_entry(const PlannedKernel& k);       // k_pr.hip: cdpr_step_kernel, per-robot handles (PR = true)
StepKernel onestep_kernel_entry(const PlannedKernel& k);       // k_onestep.hip: cdpr_onestep_kernel
StepKernel split_kernel_entry(const PlannedKernel& k);         // k_onestep.hip: cdpr_split_kernel and its steady form, cdpr_split_steady_kernel
StepKernel pair_kernel_entry(const PlannedKernel& k);          // k_pair.hip: cdpr_step_kernel_pair
StepKernel pair_stream_kernel_entry(const PlannedKernel& k);   // k_pair.hip: cdpr_pair_stream_kernel
StepKernel cable_kernel_entry(const PlannedKernel& k);         // k_cable.hip: cdpr_step_kernel_cable
GenKernel gen_step_kernel_entry(const PlannedKernel& k);       // k_gen.hip: cdpr_gen_step_kernel (its five units)
GenKernel gen_split_kernel_entry(const PlannedKernel& k);      // k_gen_split.hip: cdpr_gen_split_kernel
GenKernel gen_lean_kernel_entry(const PlannedKernel& k);       // k_gen_split.hip: cdpr_gen_lean_kernel
F64Kernel f64_step_kernel_entry(const PlannedKernel& k);       // k_f64.hip: cdpr_step_kernel_f64 (its four units)
F64Kernel f64_split_kernel_entry(const PlannedKernel& k);      // k_f64.hip: cdpr_split_kernel_f64

// The entry point of a descriptor, by argument type: nullptr for an id of another type, and where no unit instantiates it
inline StepKernel step_entry(const PlannedKernel& k) {
  switch (k.id) {
    case KernelId::StepSingle: case KernelId::StepMulti: case KernelId::Lowreg: case KernelId::PhysStep: case KernelId::Rollout: case KernelId::PhysRollout:
      return step_kernel_entry(k);
    case KernelId::PrSingle: case KernelId::PrLowreg: case KernelId::PrMulti: case KernelId::PrRollout: return pr_step_kernel_entry(k);
    case KernelId::Onestep: case KernelId::OnestepPersist: return onestep_kernel_entry(k);
    case KernelId::Split: case KernelId::PrSplit: return split_kernel_entry(k);
    case KernelId::PairSingle: case KernelId::PairMulti: return pair_kernel_entry(k);
    case KernelId::PairStream: return pair_stream_kernel_entry(k);
    case KernelId::Cable: return cable_kernel_entry(k);
    default: return nullptr;
  }
}
inline GenKernel gen_entry(const PlannedKernel& k) {
  switch (k.id) {
    case KernelId::GenOne: case KernelId::GenMulti: case KernelId::GenRollout: return gen_step_kernel_entry(k);
    case KernelId::GenSplit: return gen_split_kernel_entry(k);
    case KernelId::GenLean: return gen_lean_kernel_entry(k);
    default: return nullptr;
  }
}
inline F64Kernel f64_entry(const PlannedKernel& k) {
  switch (k.id) {
    case KernelId::F64: case KernelId::F64Pr: case KernelId::F64Tstop: case KernelId::F64Long: case KernelId::F64Hold: case KernelId::F64HoldPr:
      return f64_step_kernel_entry(k);
    case KernelId::F64Split: case KernelId::F64SplitHold: return f64_split_kernel_entry(k);
    default: return nullptr;
  }
}
// ... and whatever its type (the check for a missing instantiation, the debug exports)
inline const void* entry_address(const PlannedKernel& k) {
  if (StepKernel s = step_entry(k)) return reinterpret_cast<const void*>(s);
  if (GenKernel g = gen_entry(k)) return reinterpret_cast<const void*>(g);
  return reinterpret_cast<const void*>(f64_entry(k));
}

// Has every kernel that launches of shape `s` can take an instantiation?  A handle's mode and the role-split kernel's steady state
// change from launch to launch, so both are tried both ways.  Returns the first descriptor without one (id None: all are there).
inline PlannedKernel missing_entry(const KernelPlan& p, LaunchShape s) {
  for (const bool vel : {false, true})
    for (const bool steady : {false, true}) {
      s.vel = vel, s.split_steady = steady;
      const PlannedKernel k = planned_kernel(p, s);
      if (!entry_address(k)) return k;
    }
  return PlannedKernel{};
}
// ... and over every launch shape there is: one step or several, world step 0, a schedule, a rollout, the stream kernel's steady state
inline PlannedKernel missing_entry(const KernelPlan& p) {
  for (int shape = 0; shape < 32; ++shape) {
    LaunchShape s;
    s.steps = (shape & 1) ? 2 : 1, s.first_world = (shape & 2) != 0, s.scheduled = (shape & 4) != 0, s.rollout = (shape & 8) != 0, s.steady = (shape & 16) != 0;
    const PlannedKernel k = missing_entry(p, s);
    if (k.id != KernelId::None) return k;
  }
  return PlannedKernel{};
}

}  // namespace cdpr
