// cdpr_cem.hpp - the cross-entropy method around the MPC rollout, on the device: the command batch from a mean and a sigma plan
// (cdpr_cem_sample_device: the MPPI sampler, cdpr_mppi.hpp, instantiated with "sigma from a plan") and the refit of both plans to the
// K best samples (cdpr_cem_update_device).  Host side: cdpr_engine_cem.hip, instantiated in k_cem.hip; include/cdpr.h has the definition
// in full.  Neither kernel reads robot state.
//
// Update.  A workgroup of 256 per robot.
// Phase 1, selection, all 256 lanes strided over the S costs.  A cost folds to a key whose unsigned order is the order of the values
// (-0 first made +0; an unusable cost gets 0xFFFFFFFF, which no finite cost folds to); the keys go to LDS.  M = the usable ones,
// K' = min(K, M), the first sample of the order by two min-reductions (key, then index).  The K'-th smallest key T by a 32-round bitwise
// search: T = max {x : count(key < x) < K'}, built from the top bit down, each round a strided count by ballots (a lane's first key
// stays in a register: no LDS read up to S = 256) and the four waves' counts added (one barrier, the partial counts double-buffered).
// r = K' - count(key < T) samples with key == T are elites, the first r by index.  One more pass in ascending chunks of 256: ballots give every lane the number of smaller keys and of ties in front of it, so an elite knows its place
// lt + min(eq, r) in the ascending list of elite indices (LDS), d_elite is written, and the r-th tie's index is remembered.
// Phase 2, fit, a wave per horizon step (rounds of four steps).  Lane l takes the elites l, l + 64, .. of the list in that order, reads
// each one's row of n floats (16-byte loads where n % 4 == 0 and the buffer is aligned) and adds it up; the xor butterfly of
// cdpr_mppi.hpp; m = sum / (float)K' in every lane; the same walk again with d = v - m, fmaf(d, d, acc) - from the registers where
// K' <= 64 (a lane has at most one elite), from the cache otherwise -, the butterfly, var = sum / (float)K', f = sqrtf(var); lane i < n
// blends and stores.  Only K' * H * n floats of the robot's S * H * n are read.  The old rows of a round are read before the fit;
// under SHIFT a barrier stands between a round's reads and its writes (row t - 1 is written by the wave of row t), and no later round
// reads what an earlier one wrote.
// More samples than kCemLdsSamples: no keys and no list in LDS.  Every pass folds the costs again (the same keys), and in phase 2 lane
// l walks the SAMPLES l, l + 64, .. and adds those that are elites (key < T, or key == T and index <= the r-th tie's): the same set,
// sums in ascending index per lane.  The order of every sum is fixed by (S, K', the elite set): the same inputs give the same bits.
#pragma once
#include "cdpr_mppi.hpp"  // kMppiBlock, cost_usable, wave_sum, the sampler

namespace cdpr {

constexpr uint32_t kCemLdsSamples = 4096u;  // keys and elite list kept in LDS (16 KiB each); above: costs folded again, no list

struct CemUpdateArgs {
  const float* cost;      // float[B][S]
  const float* commands;  // float[B][H][S][n]
  float* mean;            // float[B][H][n], in/out
  float* sigma;           // float[B][H][n], in/out
  float* action;          // float[B][n] or null
  float* elite;           // float[B][S] or null
  int32_t* best;          // int32[B] or null
  uint32_t* status;       // uint32[4] or null: [0] robots updated, [1] robots degenerate, [2] bad costs, [3] robots short of K usable costs
  uint32_t batch, samples, horizon, elites;
  uint32_t shift;         // CDPR_CEM_SHIFT
  uint32_t lds_samples;   // S where keys and list are kept in LDS (S <= kCemLdsSamples), else 0
  uint32_t vec;           // 1: n % 4 == 0 and the command buffer is 16-byte aligned - 16-byte loads
  float alpha, sigma_min, sigma_max;
};

// the sortable key of a cost: finite floats order as their bits do once the sign is folded (cdpr_mppi_update_kernel), -0 as +0
CDPR_DEV uint32_t cem_key(float c) {
  if (!cost_usable(c)) return 0xFFFFFFFFu;
  uint32_t bits = __float_as_uint(c);
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// sum / minimum of one word per lane over the workgroup of four waves, the same in every lane.  xs: uint32[8] in LDS, used in halves
// by turns - one barrier per call is enough: whoever writes a half again has passed the barrier behind the last reads of it.
template <bool kMin>
CDPR_DEV uint32_t cem_block_reduce(uint32_t v, uint32_t* xs, uint32_t& turn) {
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d);
    v = kMin ? (o < v ? o : v) : v + o;
  }
  uint32_t* const x = xs + 4u * (turn & 1u);
  ++turn;
  if ((threadIdx.x & 63u) == 0u) x[threadIdx.x >> 6] = v;
  __syncthreads();
  if constexpr (kMin) {
    const uint32_t p = x[0] < x[1] ? x[0] : x[1], q = x[2] < x[3] ? x[2] : x[3];
    return p < q ? p : q;
  } else {
    return x[0] + x[1] + x[2] + x[3];
  }
}

// how many of the workgroup's lanes, over the S keys, hold a key below `bound`: ballots per chunk of 256 (the count is the same in
// every lane of a wave), the four waves' counts through xs as above.  key0: the lane's key of the first chunk, kept in a register
CDPR_DEV uint32_t cem_count_below(uint32_t bound, uint32_t key0, const uint32_t* keys, const float* cost, uint32_t S, uint32_t* xs, uint32_t& turn) {
  uint32_t cnt = (uint32_t)__popcll(__ballot(key0 < bound));
  for (uint32_t base = kMppiBlock; base < S; base += kMppiBlock) {
    const uint32_t s = base + threadIdx.x;
    const uint32_t key = s < S ? (keys ? keys[s] : cem_key(cost[s])) : 0xFFFFFFFFu;
    cnt += (uint32_t)__popcll(__ballot(key < bound));
  }
  uint32_t* const x = xs + 4u * (turn & 1u);
  ++turn;
  if ((threadIdx.x & 63u) == 0u) x[threadIdx.x >> 6] = cnt;
  __syncthreads();
  return x[0] + x[1] + x[2] + x[3];
}

// the n floats of one sample's row
template <int N>
CDPR_DEV void cem_load_row(const float* p, uint32_t vec, float (&v)[N]) {
  if constexpr (N % 4 == 0) {
    if (vec) {
#pragma unroll
      for (int i = 0; i < N; i += 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = p[i];
}

// a plan of a degenerate robot under SHIFT: one row on, the last row repeated, chunk by chunk in ascending order with a barrier
// between a chunk's reads and its writes (every thread of the workgroup calls this)
CDPR_DEV void cem_shift_plan(float* plan, size_t last /*(H - 1) * n*/, uint32_t n) {
  for (size_t base = 0u; base < last; base += kMppiBlock) {
    const size_t idx = base + threadIdx.x;
    const float v = idx < last ? plan[idx + n] : 0.0f;
    __syncthreads();
    if (idx < last) plan[idx] = v;
    __syncthreads();
  }
}

template <int N>
__global__ __launch_bounds__(kMppiBlock) void cdpr_cem_update_kernel(const CemUpdateArgs a) {
  extern __shared__ uint32_t cem_lds[];  // uint32 keys[lds_samples], list[lds_samples]
  __shared__ uint32_t xs[8], xe[16], xcut;
  const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t S = a.samples, H = a.horizon;
  const float* cost = a.cost + (size_t)b * S;
  const bool keep = a.lds_samples != 0u;
  uint32_t* const keys = cem_lds;
  uint32_t* const list = cem_lds + a.lds_samples;
  uint32_t turn = 0u;

  // keys; the usable ones counted; the least key and the lowest index that has it
  uint32_t usable = 0u, mkey = 0xFFFFFFFFu, midx = 0xFFFFFFFFu, key0 = 0xFFFFFFFFu;
  for (uint32_t base = 0u; base < S; base += kMppiBlock) {
    const uint32_t s = base + tid;
    const uint32_t key = s < S ? cem_key(cost[s]) : 0xFFFFFFFFu;
    const bool ok = key != 0xFFFFFFFFu;
    if (keep && s < S) keys[s] = key;
    if (base == 0u) key0 = key;
    usable += ok ? 1u : 0u;
    if (key < mkey) mkey = key, midx = s;  // (a lane's s ascend: the first of equal keys stays)
    if (a.status) wave_count_add(a.status + 2, s < S && !ok);
  }
  const uint32_t M = cem_block_reduce<false>(usable, xs, turn);  // (its barrier also stands between the keys' stores and their loads)
  const uint32_t least = cem_block_reduce<true>(mkey, xs, turn);
  const uint32_t first = cem_block_reduce<true>(mkey == least ? midx : 0xFFFFFFFFu, xs, turn);
  const bool degenerate = M == 0u;
  const uint32_t Kp = a.elites < M ? a.elites : M;

  float* const mean = a.mean + (size_t)b * H * N;
  float* const sigma = a.sigma + (size_t)b * H * N;
  if (tid == 0u) {
    if (a.status) {
      atomicAdd(a.status + (degenerate ? 1 : 0), 1u);
      if (!degenerate && M < a.elites) atomicAdd(a.status + 3, 1u);
    }
    if (a.best) a.best[b] = degenerate ? -1 : (int32_t)first;
  }
  if (degenerate) {  // (uniform over the workgroup) both plans stay, one row on under SHIFT; the action is the old first row
    if (a.elite)
      for (uint32_t s = tid; s < S; s += kMppiBlock) a.elite[(size_t)b * S + s] = 0.0f;
    if (a.action && tid < (uint32_t)N) a.action[(size_t)b * N + tid] = mean[tid];
    if (!a.shift) return;
    __syncthreads();  // (the action's reads are done before row 0 is written)
    cem_shift_plan(mean, (size_t)(H - 1u) * N, N);
    cem_shift_plan(sigma, (size_t)(H - 1u) * N, N);
    return;
  }

  // the K'-th smallest key: T = max {x : count(key < x) < K'}
  uint32_t T = 0u;
  for (uint32_t bit = 0x80000000u; bit != 0u; bit >>= 1) {
    const uint32_t cand = T | bit;
    if (cem_count_below(cand, key0, keep ? keys : nullptr, cost, S, xs, turn) < Kp) T = cand;
  }
  const uint32_t r = Kp - cem_count_below(T, key0, keep ? keys : nullptr, cost, S, xs, turn);  // ties to take: 1 <= r <= count(key == T)

  // places: ascending chunks, the counts in front of a lane from the ballots (T < 0xFFFFFFFF: a lane past S is neither)
  uint32_t lt_base = 0u, eq_base = 0u;
  for (uint32_t base = 0u; base < S; base += kMppiBlock) {
    const uint32_t s = base + tid;
    const uint32_t key = s < S ? (keep ? keys[s] : cem_key(cost[s])) : 0xFFFFFFFFu;
    const bool lt = key < T, eq = key == T;
    const uint64_t bl = __ballot(lt), be = __ballot(eq), front = (1ull << lane) - 1ull;
    uint32_t* const x = xe + 8u * (turn & 1u);
    ++turn;
    if (lane == 0u) x[wave] = (uint32_t)__popcll(bl), x[4u + wave] = (uint32_t)__popcll(be);
    __syncthreads();
    uint32_t ltp = lt_base + (uint32_t)__popcll(bl & front), eqp = eq_base + (uint32_t)__popcll(be & front);
#pragma unroll
    for (uint32_t w = 0u; w < 4u; ++w) {
      if (w < wave) ltp += x[w], eqp += x[4u + w];
      lt_base += x[w], eq_base += x[4u + w];
    }
    const bool is_elite = lt || (eq && eqp < r);
    if (s < S) {
      if (a.elite) a.elite[(size_t)b * S + s] = is_elite ? 1.0f : 0.0f;
      if (keep && is_elite) list[ltp + (eqp < r ? eqp : r)] = s;  // (< count(key < T) + r = K' <= S)
      if (eq && eqp + 1u == r) xcut = s;
    }
  }
  __syncthreads();
  const uint32_t cut = xcut;

  // the fit: a wave per horizon step, four steps a round
  const float* cmd = a.commands + (size_t)b * H * S * N;
  const float count = (float)Kp;
  const bool select = a.alpha == 1.0f;
  for (uint64_t t0 = 0u; t0 < H; t0 += 4u) {
    const uint64_t t = t0 + wave;
    const bool active = t < H, mine = active && lane < (uint32_t)N;
    const float old_m = mine ? mean[t * N + lane] : 0.0f, old_s = mine ? sigma[t * N + lane] : 0.0f;
    float fit_m = 0.0f, fit_v = 0.0f;
    if (active) {
      const float* row = cmd + (size_t)t * S * N;
      float v[N], acc[N], m[N];
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = 0.0f, acc[i] = 0.0f;
      if (keep) {
        for (uint32_t k = lane; k < Kp; k += 64u) {
          cem_load_row<N>(row + (size_t)list[k] * N, a.vec, v);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] += v[i];
        }
      } else {
        for (uint32_t s = lane; s < S; s += 64u) {
          const uint32_t key = cem_key(cost[s]);
          if (key < T || (key == T && s <= cut)) {
            cem_load_row<N>(row + (size_t)s * N, a.vec, v);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += v[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        m[i] = wave_sum(acc[i]) / count;
        if (lane == (uint32_t)i) fit_m = m[i];
        acc[i] = 0.0f;
      }
      if (keep) {
        for (uint32_t k = lane; k < Kp; k += 64u) {
          if (Kp > 64u) cem_load_row<N>(row + (size_t)list[k] * N, a.vec, v);  // (else: the lane's one elite is still in v)
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const float d = v[i] - m[i];
            acc[i] = fmaf(d, d, acc[i]);
          }
        }
      } else {
        for (uint32_t s = lane; s < S; s += 64u) {
          const uint32_t key = cem_key(cost[s]);
          if (key < T || (key == T && s <= cut)) {
            cem_load_row<N>(row + (size_t)s * N, a.vec, v);
#pragma unroll
            for (int i = 0; i < N; ++i) {
              const float d = v[i] - m[i];
              acc[i] = fmaf(d, d, acc[i]);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float var = wave_sum(acc[i]) / count;
        if (lane == (uint32_t)i) fit_v = var;
      }
    }
    if (a.shift) __syncthreads();  // (every wave has read its old rows: row t - 1 may be written)
    if (mine) {
      const float f = sqrtf(fit_v);
      const float new_m = select ? fit_m : fmaf(a.alpha, fit_m - old_m, old_m);
      const float new_s = fminf(fmaxf(select ? f : fmaf(a.alpha, f - old_s, old_s), a.sigma_min), a.sigma_max);
      if (t == 0u && a.action) a.action[(size_t)b * N + lane] = new_m;
      float* const out_m = mean + t * N + lane;
      float* const out_s = sigma + t * N + lane;
      if (!a.shift) {
        *out_m = new_m, *out_s = new_s;
      } else {  // out[t - 1] = plan'[t], the last row repeated
        if (t > 0u) out_m[-N] = new_m, out_s[-N] = new_s;
        if (t == H - 1u) *out_m = new_m, *out_s = new_s;
      }
    }
  }
}

using CemUpdateKernel = void (*)(const CemUpdateArgs);
CemUpdateKernel cem_update_kernel_entry(uint32_t n);  // k_cem.hip: nullptr outside 1 .. 12
MppiSampleKernel cem_sample_kernel_entry(bool vec);   // k_cem.hip: the sampler with sigma from a plan

}  // namespace cdpr
