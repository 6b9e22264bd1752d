// cdpr_resample.hpp - systematic (low-variance) resampling on the device: float weights in, the int32 source map of
// cdpr_copy_robots_device out (cdpr_resample_map_device, cdpr_resample_device; host side: cdpr_engine_resample.hip, instantiated in
// k_resample.hip).  The batch is G = B / P groups of P consecutive robots; every group is resampled on its own from one random word.
//
// The definition is in integers (include/cdpr.h has it in full), so that no result depends on the order a parallel scan adds in:
//   m      the largest usable weight (finite and > 0); none: the group is degenerate, map -1, ess 0
//   q_i    (uint64) floor((double)w_i / (double)m * 2^30) for a usable weight, else 0          Q = sum q_i, C_i its inclusive prefix
//   ess    Q * Q / (Shi * 2^30 + Slo) in double, q_i^2 = hi_i * 2^30 + lo_i; resampled iff ess < (double)gate * P
//   o      (Q * u) >> 32 (96-bit product), positions j * Q + o, j = 0 .. P - 1, against the bounds P * C_i:
//   c_i    N(P * C_i) - N(P * C_{i-1}),  N(x) = 0 for x <= o, else min(P, (x - o + Q - 1) / Q)   offspring of robot i, sum c_i = P
//   map    survivors (c_i > 0) keep their index; the k-th dead robot in index order takes the k-th extra slot in index order
//          (extras_i = max(c_i - 1, 0)): its source is the smallest i whose inclusive scan of extras exceeds k
//
// One team of lanes per group, consecutive robots per lane, three forms by group size (resample_form):
//   P <= 64      a wave per group, four groups per workgroup, one robot per lane
//   P <= 1 024   a workgroup of 256 per group, four robots per lane, the weights stay in registers
//   P <= 65 536  the same workgroup walks the group in chunks of 1 024 with carries; the weights are read once per pass (three passes:
//                maximum, sums, counts) and a dead robot's rank waits in its own map entry for the last pass
// Phases: weights -> team maximum -> quantise -> one scan of (q, hi, lo) (within a wave by cross-lane shifts, across waves through a
// few LDS words) -> counts by the closed form, one 64-bit division per bound -> one scan of the pair (extras, dead) -> the inclusive
// scan of extras into LDS, where every dead robot searches it by bisection (no loop over a robot's offspring: a one-hot group gives
// one robot P - 1 extras) -> the map, -1 included, so the caller's buffer needs no clearing.  The scan of extras never exceeds
// P - 1 <= 65 535 (sum extras = sum dead), so uint16 holds it and the largest group takes 128 KiB of the CU's 160 KiB of LDS: no
// global scratch at any size.  Control flow is uniform over the workgroup (a group that is degenerate or over the gate runs the
// same phases with nothing dead), so every barrier is met by every wave.  Counts of weights and groups go through wave_count_add; a
// group's destinations are the scan's own total, added once per group (ordinary atomicAdd, as in wave_count_add).
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_kernels.hpp"

namespace cdpr {

constexpr uint32_t kResampleBlock = 256u;   // threads of a workgroup, every form
constexpr uint32_t kResampleItems = 4u;     // consecutive robots per lane of the workgroup forms
constexpr uint32_t kResampleWaveP = 64u;    // largest group of the wave-per-group form
constexpr uint32_t kResampleOneP = kResampleBlock * kResampleItems;  // largest group whose weights stay in registers
constexpr uint32_t kResampleMaxP = 65536u;
constexpr double kResampleScale = 1073741824.0;  // 2^30

struct ResampleArgs {
  const float* weights;   // float[B]
  const uint32_t* words;  // uint32[G] or null: 2^31 for every group
  int32_t* source;        // int32[B]
  float* ess;             // float[G] or null
  uint32_t* status;       // uint32[5] or null: [0] destinations, [2] groups resampled, [3] groups degenerate, [4] bad weights
  uint32_t group, groups; // P, G
  float gate;
  uint32_t count_destinations;  // 0: status[0] is left to the copy kernel that follows (the fused call)
};

// Inclusive scan of N sums at once over a team of kTeam lanes (64: the wave, 256: the workgroup), with the team's totals.  xw: 4 * N
// LDS words of the workgroup form.  Every wave of the workgroup comes through here (two barriers in the workgroup form).
template <uint32_t kTeam, int N>
CDPR_DEV void team_scan(uint64_t (&v)[N], uint64_t (&total)[N], uint64_t* xw) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1u; d < 64u; d <<= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const uint64_t up = __shfl_up(v[k], d);
      if (lane >= d) v[k] += up;
    }
  }
  if constexpr (kTeam == 64u) {
#pragma unroll
    for (int k = 0; k < N; ++k) total[k] = __shfl(v[k], 63);
  } else {
    const uint32_t wave = threadIdx.x >> 6;
    if (lane == 63u) {
#pragma unroll
      for (int k = 0; k < N; ++k) xw[k * 4 + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
      uint64_t before = 0, all = 0;
#pragma unroll
      for (uint32_t w = 0; w < 4u; ++w) {
        const uint64_t t = xw[k * 4 + w];
        all += t;
        if (w < wave) before += t;
      }
      v[k] += before, total[k] = all;
    }
    __syncthreads();
  }
}

// ... and the team's maximum of a word
template <uint32_t kTeam>
CDPR_DEV uint32_t team_max(uint32_t v, uint32_t* xw) {
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  if constexpr (kTeam == 256u) {
    if ((threadIdx.x & 63u) == 0u) xw[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) v = xw[w] > v ? xw[w] : v;
    __syncthreads();
  }
  return v;
}

// a weight's bits: usable (finite and > 0: +denormal .. +max), bad (NaN, +-inf, negative; -0 is a zero)
CDPR_DEV bool weight_usable(uint32_t bits) { return bits - 1u < 0x7F7FFFFFu; }
CDPR_DEV bool weight_bad(uint32_t bits) { return bits >= 0x7F800000u && bits != 0x80000000u; }

// q_i: one IEEE double division, then the power of two
CDPR_DEV uint64_t quantise(float w, double m) {
  return weight_usable(__float_as_uint(w)) ? (uint64_t)floor((double)w / m * kResampleScale) : 0u;
}

template <uint32_t kTeam, uint32_t kItems, bool kOne>
__global__ __launch_bounds__(kResampleBlock) void cdpr_resample_kernel(const ResampleArgs a) {
  extern __shared__ uint16_t resample_lds[];  // the inclusive scan of extras: uint16[P] (wave form: 64 per group)
  __shared__ uint64_t xw[3 * 4];
  constexpr uint32_t kChunk = kTeam * kItems;
  const uint32_t team = threadIdx.x / kTeam, t = threadIdx.x % kTeam;
  const uint32_t g = blockIdx.x * (kResampleBlock / kTeam) + team;
  const bool have = g < a.groups;  // (wave form: the last workgroup's spare waves run on with no robot of their own)
  const uint32_t P = a.group, Pv = have ? P : 0u;
  const uint32_t span = kOne ? 1u : P;  // chunk bases: 0, kChunk, .. below span
  const size_t row = (size_t)g * P;
  uint16_t* const E = resample_lds + team * (kTeam == 64u ? 64u : 0u);

  float w[kItems];
  const auto load = [&](uint32_t base) {
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t i = base + t * kItems + j;
      w[j] = i < Pv ? a.weights[row + i] : 0.0f;
    }
  };
  if constexpr (kOne) load(0u);

  // the largest usable weight (positive floats order as their bits), the bad ones counted
  uint32_t mbits = 0u;
  for (uint32_t base = 0u; base < span; base += kChunk) {
    if constexpr (!kOne) load(base);
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t bits = __float_as_uint(w[j]);
      if (weight_usable(bits) && bits > mbits) mbits = bits;
      if (a.status) wave_count_add(a.status + 4, weight_bad(bits));
    }
  }
  mbits = team_max<kTeam>(mbits, reinterpret_cast<uint32_t*>(xw));
  const bool degenerate = mbits == 0u;
  const double m = (double)__uint_as_float(mbits);

  // Q, Shi, Slo; a group in registers keeps q and its exclusive prefix from here
  uint64_t q[kItems], cexcl = 0, Q = 0, Shi = 0, Slo = 0;
  for (uint32_t base = 0u; base < span; base += kChunk) {
    if constexpr (!kOne) load(base);
    uint64_t v[3] = {0, 0, 0}, tot[3];
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      q[j] = quantise(w[j], m);
      const uint64_t sq = q[j] * q[j];
      v[0] += q[j], v[1] += sq >> 30, v[2] += sq & 0x3FFFFFFFu;
    }
    const uint64_t own = v[0];
    team_scan<kTeam, 3>(v, tot, xw);
    cexcl = v[0] - own;
    Q += tot[0], Shi += tot[1], Slo += tot[2];
  }
  const double Qd = (double)Q;
  const double ess = degenerate ? 0.0 : (Qd * Qd) / ((double)Shi * kResampleScale + (double)Slo);
  const bool resample = !degenerate && ess < (double)a.gate * (double)P;
  if (have && t == 0u && a.ess) a.ess[g] = (float)ess;
  if (a.status && t < 64u) {
    wave_count_add(a.status + 2, have && t == 0u && resample);
    wave_count_add(a.status + 3, have && t == 0u && degenerate);
  }

  // offspring counts, the scan of (extras, dead) as one word (extras high, dead low: neither sum reaches 2^32), ranks of the dead
  const uint64_t Qs = Q ? Q : 1u;
  const uint64_t u = (have && a.words) ? a.words[g] : 0x80000000u;
  const uint64_t o = (__umul64hi(Q, u) << 32) | ((Q * u) >> 32);
  const auto below = [&](uint64_t x) -> uint64_t {  // N(x): positions under the bound x
    if (x <= o) return 0u;
    const uint64_t n = (x - o + Qs - 1u) / Qs;
    return n < P ? n : P;
  };
  int32_t rank[kItems];
  uint64_t ccarry = 0, pcarry = 0;
  for (uint32_t base = 0u; base < span; base += kChunk) {
    if constexpr (!kOne) {
      load(base);
      uint64_t v[1] = {0}, tot[1];
#pragma unroll
      for (uint32_t j = 0; j < kItems; ++j) q[j] = quantise(w[j], m), v[0] += q[j];
      const uint64_t own = v[0];
      team_scan<kTeam, 1>(v, tot, xw);
      cexcl = ccarry + v[0] - own;
      ccarry += tot[0];
    }
    uint64_t C = cexcl, nprev = below(P * C), pair[kItems], acc[1] = {0}, tot[1];
    bool dead[kItems];
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      C += q[j];
      const uint64_t n = below(P * C), c = n - nprev;
      nprev = n;
      dead[j] = resample && base + t * kItems + j < Pv && c == 0u;
      acc[0] += ((resample && c > 1u ? c - 1u : 0u) << 32) | (dead[j] ? 1u : 0u);
      pair[j] = acc[0];
    }
    const uint64_t own = acc[0];
    team_scan<kTeam, 1>(acc, tot, xw);
    const uint64_t pexcl = pcarry + acc[0] - own;
    pcarry += tot[0];
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t i = base + t * kItems + j;
      const uint64_t incl = pexcl + pair[j];
      rank[j] = dead[j] ? (int32_t)((uint32_t)incl - 1u) : -1;
      if (i < Pv) {
        E[i] = (uint16_t)(incl >> 32);
        if constexpr (!kOne) a.source[row + i] = rank[j];
      }
    }
  }
  // the group's destinations: the scan's own total of the dead, one add per group
  if (a.status && a.count_destinations && have && t == 0u && (uint32_t)pcarry != 0u) atomicAdd(a.status, (uint32_t)pcarry);
  __syncthreads();

  // the map: the k-th dead robot takes the smallest i whose inclusive scan of extras exceeds k
  for (uint32_t base = 0u; base < span; base += kChunk) {
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t i = base + t * kItems + j;
      if (i >= Pv) continue;
      const int32_t k = kOne ? rank[j] : a.source[row + i];
      if (k < 0) {
        if constexpr (kOne) a.source[row + i] = -1;
        continue;
      }
      uint32_t lo = 0u, hi = P;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t)E[mid] > (uint32_t)k) hi = mid;
        else lo = mid + 1u;
      }
      a.source[row + i] = (int32_t)(row + lo);
    }
  }
}

// which form serves a group size, and what a launch of it takes
struct ResampleForm {
  void (*kernel)(const ResampleArgs);
  uint32_t groups_per_block;
  size_t lds;  // dynamic LDS bytes
};
ResampleForm resample_form(uint32_t P);  // k_resample.hip

}  // namespace cdpr
