// cdpr_mppi.hpp - MPPI around the MPC rollout, on the device: the perturbed command batch from a nominal plan
// (cdpr_mppi_sample_device) and the rollout's costs folded into the next plan (cdpr_mppi_update_device).  Host side:
// cdpr_engine_mppi.hip, instantiated in k_mppi.hip; include/cdpr.h has the definition in full.  Neither kernel reads robot state.
//
// Sample.  Robot b (global index g = robot_offset + b, modulo 2^32) owns E = H * S * n consecutive floats of d_commands, element
// e = (t * S + s) * n + i.  One thread per group j = e >> 2 of four elements: Philox4x32-10 on the counter (j, g, iteration, 0) under
// the key (seed_lo, seed_hi) gives four words, two Box-Muller pairs give four normals, v = fmaf(sigma, z_k, U[b][t][i]), clamped where
// asked, the nominal itself at s = 0 where asked.  E a multiple of 4 and a 16-byte aligned buffer: one 16-byte store per thread;
// otherwise four guarded dword stores (the last group of a robot is partial when E is no multiple of 4).  A workgroup of 256 is
// 256 >> k robots of 2^k lanes each (k chosen by the host so that 2^k >= min(groups per robot, 256)), so small plans fill their
// waves; blockIdx.x walks a robot's groups, blockIdx.y and .z the robots.  The nominal row is read through the cache (S * n
// consecutive elements share one row of n floats).
//
// Update.  A workgroup of 256 per robot.  Phase 1, all 256 lanes strided over the S costs: the least finite cost (order-free), then
// w_s = expf((c_min - c_s) / temperature) into LDS (and d_weights), eta = sum w and sum w^2 per lane in ascending s, a fixed xor
// butterfly over the wave, the four waves' sums added in wave order.  Phase 2, one wave per horizon step t (t = wave, wave + 4, ..):
// lane l walks the samples s = l, l + 64, .. in ascending order, reads the n contiguous floats of (t, s), keeps n partial sums
// (fmaf, a weight of exactly 0 selected out), the same butterfly, lane i < n divides by eta and stores.  The order of every sum is
// fixed: the same inputs give the same bits on every run.  More samples than the LDS array holds (kMppiLdsSamples): phase 2 takes
// w_s from the cost again, by the same expression - the same bits.  No robot row of d_nominal is read outside the degenerate case
// (U' is a function of the commands), and there the shifted copy goes chunk by chunk in ascending order with a barrier between a
// chunk's reads and its writes: every element is read before it is overwritten.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_step_kernel.hpp"  // CDPR_DEV, wave_count_add

namespace cdpr {

constexpr uint32_t kMppiBlock = 256u;
constexpr uint32_t kMppiLdsSamples = 8192u;  // weights kept in LDS (32 KiB); above: recomputed from the cost in phase 2

struct MppiSampleArgs {
  const float* nominal;  // float[B][H][n]
  float* commands;       // float[B][H][S][n]
  uint64_t elems;        // E = H * S * n
  uint64_t row;          // S * n
  uint32_t batch, samples, horizon, n;
  uint32_t lane_shift;   // k: 2^k lanes of a workgroup per robot
  uint32_t flags;
  float sigma, lo, hi;
  float inv_n, inv_samples;  // 1 / n, 1 / S rounded to float
  uint32_t key0, key1, iteration, robot_offset;
  const float* sigma_plan;  // float[B][H][n]: the kPlan instantiations (cdpr_cem_sample_device) take sigma from here, entry by entry
};

struct MppiUpdateArgs {
  const float* cost;      // float[B][S]
  const float* commands;  // float[B][H][S][n]
  float* nominal;         // float[B][H][n], in/out
  float* action;          // float[B][n] or null
  float* weights;         // float[B][S] or null
  float* ess;             // float[B] or null
  uint32_t* status;       // uint32[3] or null: [0] robots updated, [1] robots degenerate, [2] bad costs
  uint32_t batch, samples, horizon;
  uint32_t shift;         // CDPR_MPPI_SHIFT
  uint32_t lds_samples;   // min(S, kMppiLdsSamples) where the weights are kept in LDS, else 0
  uint32_t vec;           // 1: n % 4 == 0 and the command buffer is 16-byte aligned - 16-byte loads
  float temperature;
};

// Philox4x32-10 (Salmon et al., SC'11): the published multipliers and key increments
CDPR_DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];  // (one 32 x 32 -> 64 multiply each)
    c[0] = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, c[1] = (uint32_t)p1, c[2] = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// one Box-Muller pair from two words: u1 in (0, 1], a in [0, 2), both exact in float
CDPR_DEV void box_muller(uint32_t x, uint32_t y, float& z0, float& z1) {
  const float u1 = (float)((x >> 9) + 1u) * 0x1p-23f;
  const float a = (float)(y >> 8) * 0x1p-23f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(a, &s, &c);
  z0 = r * c, z1 = r * s;
}

// kVec: E % 4 == 0 and the buffer is 16-byte aligned - one 16-byte store per group.  kPlan: sigma is a plan float[B][H][n] beside the
// nominal one and read the same way (CEM: cdpr_cem.hpp); the streams, the element order and everything else are the same
template <bool kVec, bool kPlan = false>
__global__ __launch_bounds__(kMppiBlock) void cdpr_mppi_sample_kernel(const MppiSampleArgs a) {
  const uint32_t k = a.lane_shift;
  const uint32_t sub = threadIdx.x >> k, lane = threadIdx.x & ((1u << k) - 1u);
  const uint64_t b64 = ((uint64_t)blockIdx.z * gridDim.y + blockIdx.y) * (kMppiBlock >> k) + sub;
  const uint64_t j64 = ((uint64_t)blockIdx.x << k) + lane;
  const uint64_t e0 = j64 << 2;
  if (b64 >= a.batch || e0 >= a.elems) return;
  const uint32_t b = (uint32_t)b64, j = (uint32_t)j64;  // (E <= 2^34: j < 2^32)

  uint32_t x[4] = {j, a.robot_offset + b, a.iteration, 0u};
  philox4x32_10(x, a.key0, a.key1);
  float z[4];
  box_muller(x[0], x[1], z[0], z[1]);
  box_muller(x[2], x[3], z[2], z[3]);

  // (t, s, i) of the group's first element; the other three follow by carries.  The integer divisions are of the workgroup's first
  // element, the same in every lane (scalar unit); a lane is at most 1 020 elements further on, and
  // floor(x / d) = (uint32_t)((x + 0.5) * (1 / d)) in float for x < 4 096: (x + 0.5) / d is at least 0.5 / d away from an integer and
  // the product's error is below 2^-11 / d.
  uint32_t t, s, i;
  const uint64_t base = ((uint64_t)blockIdx.x << k) << 2;
  if (a.elems <= 0xFFFFFFFFull) {  // (then S * n fits a word too)
    const uint32_t e = (uint32_t)base, row = (uint32_t)a.row;
    t = e / row;
    const uint32_t r = e - t * row;
    s = r / a.n, i = r - s * a.n;
  } else {
    t = (uint32_t)(base / a.row);
    const uint64_t r = base - (uint64_t)t * a.row;
    s = (uint32_t)(r / a.n), i = (uint32_t)(r - (uint64_t)s * a.n);
  }
  {
    const uint32_t x = i + (lane << 2);  // < 12 + 1 024
    const uint32_t ds = (uint32_t)(((float)x + 0.5f) * a.inv_n);
    i = x - ds * a.n;
    const uint32_t y = s + ds;           // < S + 1 036
    const uint32_t dt = a.samples >= 2048u ? (y >= a.samples ? 1u : 0u) : (uint32_t)(((float)y + 0.5f) * a.inv_samples);
    s = y - dt * a.samples, t += dt;
  }
  const float* u = a.nominal + ((size_t)b * a.horizon + t) * a.n;
  const float* sg = kPlan ? a.sigma_plan + ((size_t)b * a.horizon + t) * a.n : nullptr;
  const bool clamp = (a.flags & CDPR_MPPI_CLAMP) != 0u, first = (a.flags & CDPR_MPPI_NOMINAL_FIRST) != 0u;
  float v[4];
  bool in[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    in[q] = e0 + (uint64_t)q < a.elems;
    const float nom = in[q] ? u[i] : 0.0f;
    float sigma = a.sigma;
    if constexpr (kPlan) sigma = in[q] ? sg[i] : 0.0f;
    float c = (first && s == 0u) ? nom : fmaf(sigma, z[q], nom);
    if (clamp) c = fminf(fmaxf(c, a.lo), a.hi);
    v[q] = c;
    if (++i == a.n) {
      i = 0u;
      if (++s == a.samples) {  // (the next horizon step's row)
        s = 0u, u += a.n;
        if constexpr (kPlan) sg += a.n;
      }
    }
  }
  float* out = a.commands + (size_t)b * a.elems + e0;
  if constexpr (kVec) {
    *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (in[q]) out[q] = v[q];
  }
}

// a cost's weight: usable iff finite; one float subtraction, one float division, expf
CDPR_DEV bool cost_usable(float c) { return (__float_as_uint(c) & 0x7FFFFFFFu) < 0x7F800000u; }
CDPR_DEV float mppi_weight(float c, float cmin, float temperature) { return cost_usable(c) ? expf((cmin - c) / temperature) : 0.0f; }

// the wave's sum by a fixed xor butterfly (every lane ends with the same bits)
CDPR_DEV float wave_sum(float v) {
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <int N>
__global__ __launch_bounds__(kMppiBlock) void cdpr_mppi_update_kernel(const MppiUpdateArgs a) {
  extern __shared__ float mppi_w[];  // float[lds_samples]
  __shared__ float xw[2 * 4];
  __shared__ uint32_t xm[4];
  const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t S = a.samples, H = a.horizon;
  const float* cost = a.cost + (size_t)b * S;
  const bool keep = a.lds_samples != 0u;

  // the least usable cost: finite floats order as their bits do once the sign is folded (negative: all bits flipped; else: sign set)
  uint32_t mkey = 0xFFFFFFFFu;
  for (uint32_t base = 0u; base < S; base += kMppiBlock) {
    const uint32_t s = base + tid;
    const float c = s < S ? cost[s] : 0.0f;
    const bool ok = s < S && cost_usable(c);
    const uint32_t bits = __float_as_uint(c);
    const uint32_t key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    if (ok && key < mkey) mkey = key;
    if (a.status) wave_count_add(a.status + 2, s < S && !ok);
  }
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) {
    const uint32_t o = __shfl_xor(mkey, d);
    mkey = o < mkey ? o : mkey;
  }
  if (lane == 0u) xm[wave] = mkey;
  __syncthreads();
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) mkey = xm[w] < mkey ? xm[w] : mkey;
  const bool degenerate = mkey == 0xFFFFFFFFu;  // (no finite cost folds to all ones: that is a NaN's pattern)
  const float cmin = __uint_as_float((mkey & 0x80000000u) ? (mkey & 0x7FFFFFFFu) : ~mkey);

  float* nominal = a.nominal + (size_t)b * H * N;
  if (tid == 0u) {
    if (a.status) atomicAdd(a.status + (degenerate ? 1 : 0), 1u);
    if (a.ess && degenerate) a.ess[b] = 0.0f;
  }
  if (degenerate) {  // (uniform over the workgroup) U' is the old nominal: weights 0, the action its first row, the plan shifted in place
    if (a.weights)
      for (uint32_t s = tid; s < S; s += kMppiBlock) a.weights[(size_t)b * S + s] = 0.0f;
    if (a.action && tid < (uint32_t)N) a.action[(size_t)b * N + tid] = nominal[tid];
    if (!a.shift) return;
    __syncthreads();  // (the action's reads are done before row 0 is written)
    const size_t last = (size_t)(H - 1u) * N;
    for (size_t base = 0u; base < last; base += kMppiBlock) {  // (the last row repeats itself: it stays)
      const size_t idx = base + tid;
      const float v = idx < last ? nominal[idx + N] : 0.0f;
      __syncthreads();
      if (idx < last) nominal[idx] = v;
      __syncthreads();
    }
    return;
  }

  // weights, eta and sum w^2
  float eta = 0.0f, sq = 0.0f;
  for (uint32_t s = tid; s < S; s += kMppiBlock) {
    const float w = mppi_weight(cost[s], cmin, a.temperature);
    if (keep) mppi_w[s] = w;
    if (a.weights) a.weights[(size_t)b * S + s] = w;
    eta += w, sq = fmaf(w, w, sq);
  }
  eta = wave_sum(eta), sq = wave_sum(sq);
  if (lane == 0u) xw[wave] = eta, xw[4 + wave] = sq;
  __syncthreads();
  eta = ((xw[0] + xw[1]) + xw[2]) + xw[3];
  sq = ((xw[4] + xw[5]) + xw[6]) + xw[7];
  if (tid == 0u && a.ess) a.ess[b] = (eta * eta) / sq;

  // the plan: a wave per horizon step
  const float* cmd = a.commands + (size_t)b * H * S * N;
  for (uint32_t t = wave; t < H; t += 4u) {
    float acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0f;
    const float* row = cmd + (size_t)t * S * N;
    for (uint32_t s = lane; s < S; s += 64u) {
      const float w = keep ? mppi_w[s] : mppi_weight(cost[s], cmin, a.temperature);
      float v[N];
      const float* p = row + (size_t)s * N;
      if constexpr (N % 4 == 0) {
        if (a.vec) {
#pragma unroll
          for (int i = 0; i < N; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(p + i);
            v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < N; ++i) v[i] = p[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
      }
      if (w != 0.0f) {  // selected out, not multiplied: a non-finite command behind a zero weight does not reach the plan
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = fmaf(w, v[i], acc[i]);
      }
    }
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float total = wave_sum(acc[i]);
      if (lane == (uint32_t)i) mine = total;
    }
    if (lane < (uint32_t)N) {
      const float u = mine / eta;
      if (t == 0u && a.action) a.action[(size_t)b * N + lane] = u;
      float* const out = nominal + (size_t)t * N + lane;
      if (!a.shift) {
        *out = u;
      } else {  // out[t - 1] = U'[t], the last row repeated
        if (t > 0u) out[-N] = u;
        if (t == H - 1u) *out = u;
      }
    }
  }
}

using MppiUpdateKernel = void (*)(const MppiUpdateArgs);
MppiUpdateKernel mppi_update_kernel_entry(uint32_t n);  // k_mppi.hip: nullptr outside 1 .. 12
using MppiSampleKernel = void (*)(const MppiSampleArgs);
MppiSampleKernel mppi_sample_kernel_entry(bool vec);    // k_mppi.hip

constexpr uint64_t kMppiMaxElems = 1ull << 34;  // E = H * S * n: a group index is one Philox counter word
constexpr uint64_t kMppiMaxTraj = 1ull << 30;   // B * S: the rollout's own limit

// the sampler's launch (host): fills the shape, the reciprocals and lane_shift of `a` from (B, S, H, n) - E = H * S * n within
// kMppiMaxElems - and returns the grid; what is sampled around what (nominal, sigma or sigma_plan, flags, bounds, key) is the caller's
inline dim3 mppi_sample_geometry(MppiSampleArgs& a, uint32_t batch, uint32_t samples, uint32_t horizon, uint32_t n) {
  a.batch = batch, a.samples = samples, a.horizon = horizon, a.n = n;
  a.row = (uint64_t)samples * n, a.elems = (uint64_t)horizon * a.row;
  a.inv_n = 1.0f / (float)n, a.inv_samples = 1.0f / (float)samples;
  const uint64_t groups = (a.elems + 3u) / 4u;  // per robot
  uint32_t k = 0u;
  while (k < 8u && (1ull << k) < groups) ++k;
  a.lane_shift = k;
  const uint64_t robot_blocks = ((uint64_t)batch + (kMppiBlock >> k) - 1u) / (kMppiBlock >> k);
  const uint32_t gy = (uint32_t)(robot_blocks < 32768u ? robot_blocks : 32768u);
  return dim3((uint32_t)((groups + (1ull << k) - 1u) >> k), gy, (uint32_t)((robot_blocks + gy - 1u) / gy));
}
inline bool mppi_sample_vec(uint64_t elems, const float* commands) { return elems % 4u == 0u && reinterpret_cast<uintptr_t>(commands) % 16u == 0u; }

}  // namespace cdpr
