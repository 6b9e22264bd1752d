// cdpr_env.hpp — the environment view (cdpr_observe_device, cdpr_env_evaluate_device): the batch's observation tensor float[B][ld], a
// tracking reward float[B] and the verdict of a done rule, in ONE launch that loads every platform and observable row once.  A pure
// function of what the getters return at that point of the stream, as the done rules (cdpr_done.hpp, whose done_reason and done_store
// give the verdict here): nothing of the handle is written.  Two kernels, one per platform layout: the float4 slot rows of the fp32
// handles (state slots 0-4, observable slots 3 and 4 .. 4 + 3 G - 1 serve both controller paths) and the double rows of the
// precision = 64 handles.  gfx950 only; plain C++, explicit fma.
//
// One thread per robot, kEnvBlock = 128 per workgroup; every load row * stride + r, so the 64 robots of a wave read whole rows (1 KiB
// per float4 slot).  The tensor is robot-major, so the transposition goes through LDS: each thread parks its robot's columns in row t
// of a tile float[128][pitch]; behind a barrier the workgroup streams the tile out, one thread per output float, element e = row *
// width + col of the workgroup's 128 x width block going to thread e mod 128: a wave stores 64 consecutive floats, 256 contiguous bytes
// where ld = width (a run breaks only where a row ends and ld > width).
//
// Pitch = width | 1, the next odd number.  Parking is ds_write_b32 (or ds_write2_b32, two of them), whose bank is (address / 4) mod 32
// and whose conflict groups are the two 32-lane halves: the lanes of a half write t * pitch + col for 32 consecutive t and one col, and
// an odd pitch is a unit modulo 32, so the 32 addresses fall on 32 different banks - conflict-free.  (An even width as pitch would put
// lanes t and t + 16 - or closer - on one bank.)  Streaming is ds_read_b32, same banks and groups: the lanes of a half read e + (pitch -
// width) * row for 32 consecutive e.  Odd width: the pad is 0, the addresses are consecutive, conflict-free.  Even width: two lanes
// meet on a bank only if (e2 - e1) + (row2 - row1) = 32, i.e. one 2-way pair per row end inside the half - at width >= 32 at most one
// pair, one extra LDS cycle per 32 floats streamed.  The row select (live and, with a row mask, chosen) sits behind the tile, one word
// per robot; the lanes of a half read at most 1 + 31 / width different words of it, the equal ones broadcast.
//
// LDS per workgroup: (128 * pitch + 128) * 4 bytes, dynamic - 30 720 B at the widest observation, D = 3 * 12 + 22 = 58 columns (pitch
// 59): five workgroups fit in a CU's 160 KiB; none is allocated when no observation is asked for.  No scratch: the loops over cables
// index no register array.
//
// The reward and the verdict are skipped wave-uniformly by the argument's pointers (one kernel per layout serves cdpr_observe_device,
// cdpr_env_evaluate_device and every subset of its outputs), as the done kernels mask their disabled tests by `enable`.  Lanes past
// the batch read robot B - 1 and store nothing; the counts go through done_store.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_kernels.hpp"
#define CDPR_DONE_NO_KERNELS
#include "cdpr_done.hpp"

namespace cdpr {

constexpr int kEnvBlock = 128;
constexpr int kEnvFields = 8;  // CDPR_OBS_* bits 0 .. 7
constexpr uint32_t kEnvKnownFields = 0xFFu;
constexpr uint32_t kEnvFkFields = CDPR_OBS_FK_POSE | CDPR_OBS_FK_RESIDUAL;
enum EnvWeight { kEnvWPosition = 0, kEnvWOrientation, kEnvWSpeed, kEnvWRate, kEnvWEffort, kEnvWResidual, kEnvWeights };

// columns of field bit k on a handle of n cables
__host__ __device__ constexpr uint32_t env_field_width(int k, uint32_t n) { return k == 0 || k == 5 ? 7u : k == 1 ? 6u : k >= 6 ? 1u : n; }
__host__ __device__ constexpr uint32_t env_pitch(uint32_t width) { return width | 1u; }
__host__ __device__ constexpr size_t env_lds_bytes(uint32_t width) { return ((size_t)kEnvBlock * env_pitch(width) + kEnvBlock) * sizeof(float); }

// what both layouts share of the arguments
struct EnvView {
  cdpr_done_rule_t rule;
  float w[kEnvWeights];
  float alive, done_penalty;
  float home[7];                  // the target where `target` is null
  const float* target;            // float[B][7], or nullptr
  const uint8_t* row_mask;        // uint8[B], or nullptr = every row
  float* obs;                     // float[B][ld], or nullptr
  float* reward;                  // float[B], or nullptr
  DoneOut out;                    // out.mask null: no verdict is stored
  const uint32_t* episode_start;  // uint32[B]
  size_t stride;
  uint32_t batch, n;
  uint32_t step;                  // low word of the world-step counter at the call
  uint32_t fields, width, ld;
  uint32_t verdict;               // the reason word is needed: stored, or behind done_penalty
  uint8_t col[kEnvFields];        // the field table: first column of field bit k (the field's rows follow from the layout and n)
};

// a robot as the view takes it, in the precision of the handle
template <typename T>
struct EnvRobot {
  DoneInputs<T> s;
  T fk[7];  // the FK estimate (loaded where CDPR_OBS_FK_POSE asks for it)
};

// the fixed columns of the robot's tile row
template <typename T>
CDPR_DEV void env_park(const EnvView& v, float* mine, const EnvRobot<T>& q) {
  if (v.fields & CDPR_OBS_POSE) {
#pragma unroll
    for (int i = 0; i < 7; ++i) mine[v.col[0] + i] = (float)q.s.p[i];
  }
  if (v.fields & CDPR_OBS_TWIST) {
#pragma unroll
    for (int i = 0; i < 6; ++i) mine[v.col[1] + i] = (float)q.s.t[i];
  }
  if (v.fields & CDPR_OBS_FK_POSE) {
#pragma unroll
    for (int i = 0; i < 7; ++i) mine[v.col[5] + i] = (float)q.fk[i];
  }
  if (v.fields & CDPR_OBS_FK_RESIDUAL) mine[v.col[6]] = (float)q.s.fk_residual;
  if (v.fields & CDPR_OBS_AGE) mine[v.col[7]] = (float)q.s.age;
}

// the reward of include/cdpr.h, term by term in its order; `c`: the robot whose target row is read, ee: the effort chain
template <typename T>
CDPR_DEV T env_reward(const EnvView& v, const EnvRobot<T>& q, uint32_t c, T ee, uint32_t reason) {
  T g[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) g[i] = (T)(v.target ? v.target[(size_t)c * 7u + i] : v.home[i]);
  const T* const p = q.s.p;
  const T* const t = q.s.t;
  const T e0 = p[0] - g[0], e1 = p[1] - g[1], e2 = p[2] - g[2];
  const T pos = done_fma(e2, e2, done_fma(e1, e1, e0 * e0));
  const T cc = done_fma(p[6], g[6], done_fma(p[5], g[5], done_fma(p[4], g[4], p[3] * g[3])));
  const T qq = done_fma(p[6], p[6], done_fma(p[5], p[5], done_fma(p[4], p[4], p[3] * p[3])));
  const T tt = done_fma(g[6], g[6], done_fma(g[5], g[5], done_fma(g[4], g[4], g[3] * g[3])));
  const T ori = (T)1 - (cc * cc) / (qq * tt);
  const T vv = done_fma(t[2], t[2], done_fma(t[1], t[1], t[0] * t[0]));
  const T ww = done_fma(t[5], t[5], done_fma(t[4], t[4], t[3] * t[3]));
  const T term[kEnvWeights] = {pos, ori, vv, ww, ee, q.s.fk_residual};
  T r = (T)v.alive;
#pragma unroll
  for (int k = 0; k < kEnvWeights; ++k)
    if (v.w[k] != 0.0f) r = done_fma(-(T)v.w[k], term[k], r);  // (wave-uniform: a weight of 0 selects its term out)
  return reason ? r - (T)v.done_penalty : r;
}

// reward and verdict of a loaded robot; every lane of the wave arrives here (done_store ballots)
template <typename T>
CDPR_DEV void env_judge(const EnvView& v, const EnvRobot<T>& q, uint32_t r, uint32_t c, bool live, T ee) {
  const uint32_t reason = v.verdict ? done_reason(v.rule, q.s) : 0u;
  if (v.reward) {
    const T rw = env_reward(v, q, c, ee, reason);
    if (live) v.reward[r] = (float)rw;
  }
  if (v.out.mask) done_store(v.out, v.rule.enable, r, live, reason);
}

// The tile goes out: thread t takes the elements t, t + 128, ... of the workgroup's 128 x width block, (row, col) moved on by 128 =
// dq * width + dr without a division per element.  sel[row]: the row is inside the batch and chosen by the row mask.
CDPR_DEV void env_stream(const EnvView& v, const float* tile, const uint32_t* sel, uint32_t t, size_t first_robot) {
  const uint32_t width = v.width, pitch = env_pitch(width), total = (uint32_t)kEnvBlock * width;
  const uint32_t dq = (uint32_t)kEnvBlock / width, dr = (uint32_t)kEnvBlock - dq * width;
  uint32_t row = t / width, col = t - row * width;
  for (uint32_t e = t; e < total; e += (uint32_t)kEnvBlock) {  // (row = e / width < 128 here)
    if (sel[row]) v.obs[(first_robot + row) * v.ld + col] = tile[row * pitch + col];
    row += dq, col += dr;
    if (col >= width) col -= width, ++row;
  }
}

// fp32 handles, both controller paths: state slots 0-3 = [x y z qx | qy qz qw vx | vy vz wx wy | wz fk0 fk1 fk2], slot 4 = fk3 .. fk6;
// observable slot 3 = [wz | fk residual | fk iterations | flags], joint field f (0 position, 1 velocity, 2 effort) of cable i in slot
// 4 + f G + i / 4, component i % 4, G = joint_groups(n): all of the last published step
struct EnvArgs {
  EnvView view;
  const float4* state;
  const float4* obs_rows;
};

template <int kBlock>
__global__ __launch_bounds__(kBlock) void cdpr_env_kernel(const EnvArgs a) {
  static_assert(kBlock == kEnvBlock, "the tile and env_stream are laid out for kEnvBlock robots");
  extern __shared__ float env_tile[];
  const EnvView& v = a.view;
  const uint32_t t = threadIdx.x, r = blockIdx.x * (uint32_t)kBlock + t;
  const bool live = r < v.batch;
  const uint32_t c = live ? r : v.batch - 1u;
  const size_t st = v.stride;
  const bool park = v.obs != nullptr;
  float* const mine = env_tile + t * env_pitch(v.width);
  const float4 s0 = a.state[0 * st + c], s1 = a.state[1 * st + c], s2 = a.state[2 * st + c], s3 = a.state[3 * st + c];
  const float4 o3 = a.obs_rows[3 * st + c];
  EnvRobot<float> q;
  q.s.p[0] = s0.x, q.s.p[1] = s0.y, q.s.p[2] = s0.z, q.s.p[3] = s0.w, q.s.p[4] = s1.x, q.s.p[5] = s1.y, q.s.p[6] = s1.z;
  q.s.t[0] = s1.w, q.s.t[1] = s2.x, q.s.t[2] = s2.y, q.s.t[3] = s2.z, q.s.t[4] = s2.w, q.s.t[5] = s3.x;
  q.s.fk_residual = o3.y;
  q.s.flags = (uint32_t)(int)o3.w;  // (as cdpr_done_kernel)
  q.s.age = v.step - v.episode_start[c];
  q.fk[0] = s3.y, q.fk[1] = s3.z, q.fk[2] = s3.w;
  if (park && (v.fields & CDPR_OBS_FK_POSE)) {  // (slot 4 exists on handles with CDPR_STAGE_FK, which the field needs)
    const float4 s4 = a.state[4 * st + c];
    q.fk[3] = s4.x, q.fk[4] = s4.y, q.fk[5] = s4.z, q.fk[6] = s4.w;
  } else {
    q.fk[3] = q.fk[4] = q.fk[5] = q.fk[6] = 0.0f;
  }
  // the joint slots: each is loaded once, parked where its field is asked for, and the efforts go into the reward's chain
  const uint32_t n = v.n, G = (n + 3u) / 4u;
  const bool want_effort = v.reward != nullptr && v.w[kEnvWEffort] != 0.0f;
  float ee = 0.0f;  // (fma(e0, e0, 0) is e0 e0: the chain starts at cable 0)
  for (uint32_t f = 0; f < 3u; ++f) {
    const bool parked = park && ((v.fields >> (2u + f)) & 1u);
    if (!parked && !(f == 2u && want_effort)) continue;
    const uint32_t col0 = v.col[2u + f];
    for (uint32_t g = 0; g < G; ++g) {
      const float4 x = a.obs_rows[(size_t)(4u + f * G + g) * st + c];
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k) {
        if (4u * g + k >= n) continue;  // (the last group's spare components are no cable's)
        if (parked) mine[col0 + 4u * g + k] = xs[k];
        if (f == 2u) ee = fmaf(xs[k], xs[k], ee);
      }
    }
  }
  env_judge(v, q, r, c, live, ee);
  if (park) {
    uint32_t* const sel = reinterpret_cast<uint32_t*>(env_tile + (uint32_t)kBlock * env_pitch(v.width));
    env_park(v, mine, q);
    sel[t] = (live && (!v.row_mask || v.row_mask[c] != 0)) ? 1u : 0u;
    __syncthreads();
    env_stream(v, env_tile, sel, t, (size_t)blockIdx.x * (size_t)kBlock);
  }
}

// precision = 64 handles: state rows kF64Pose + 0..6, kF64Twist + 0..5, kF64StateFk + 0..6; observable rows kF64ObsResidual,
// kF64ObsFlags and kF64ObsJoint + f n + i.  Every column is the double rounded once, as the float getters hand it out; the reward is
// computed on the doubles (the residual as cdpr_get_fk_state rounds it, as the done rules take it).
struct EnvF64Args {
  EnvView view;
  const double* state;
  const double* obs_rows;
};

template <int kBlock>
__global__ __launch_bounds__(kBlock) void cdpr_env_f64_kernel(const EnvF64Args a) {
  static_assert(kBlock == kEnvBlock, "the tile and env_stream are laid out for kEnvBlock robots");
  extern __shared__ float env_tile[];
  const EnvView& v = a.view;
  const uint32_t t = threadIdx.x, r = blockIdx.x * (uint32_t)kBlock + t;
  const bool live = r < v.batch;
  const uint32_t c = live ? r : v.batch - 1u;
  const size_t st = v.stride;
  const bool park = v.obs != nullptr;
  float* const mine = env_tile + t * env_pitch(v.width);
  const double* const S = a.state + c;
  const double* const O = a.obs_rows + c;
  EnvRobot<double> q;
#pragma unroll
  for (int i = 0; i < 7; ++i) q.s.p[i] = S[(size_t)(kF64Pose + i) * st];
#pragma unroll
  for (int i = 0; i < 6; ++i) q.s.t[i] = S[(size_t)(kF64Twist + i) * st];
  q.s.fk_residual = (double)(float)O[(size_t)kF64ObsResidual * st];  // (as cdpr_done_f64_kernel)
  q.s.flags = (uint32_t)(int32_t)O[(size_t)kF64ObsFlags * st];
  q.s.age = v.step - v.episode_start[c];
  const bool fk = park && (v.fields & CDPR_OBS_FK_POSE);
#pragma unroll
  for (int i = 0; i < 7; ++i) q.fk[i] = fk ? S[(size_t)(kF64StateFk + i) * st] : 0.0;
  const uint32_t n = v.n;
  const bool want_effort = v.reward != nullptr && v.w[kEnvWEffort] != 0.0f;
  double ee = 0.0;
  for (uint32_t f = 0; f < 3u; ++f) {
    const bool parked = park && ((v.fields >> (2u + f)) & 1u);
    if (!parked && !(f == 2u && want_effort)) continue;
    const uint32_t col0 = v.col[2u + f];
    for (uint32_t i = 0; i < n; ++i) {
      const double x = O[(size_t)((uint32_t)kF64ObsJoint + f * n + i) * st];
      if (parked) mine[col0 + i] = (float)x;
      if (f == 2u) ee = fma(x, x, ee);
    }
  }
  env_judge(v, q, r, c, live, ee);
  if (park) {
    uint32_t* const sel = reinterpret_cast<uint32_t*>(env_tile + (uint32_t)kBlock * env_pitch(v.width));
    env_park(v, mine, q);
    sel[t] = (live && (!v.row_mask || v.row_mask[c] != 0)) ? 1u : 0u;
    __syncthreads();
    env_stream(v, env_tile, sel, t, (size_t)blockIdx.x * (size_t)kBlock);
  }
}

using EnvKernel = void (*)(const EnvArgs);
using EnvF64Kernel = void (*)(const EnvF64Args);
EnvKernel pick_env_kernel();         // k_env.hip
EnvF64Kernel pick_env_f64_kernel();  // k_env.hip

}  // namespace cdpr
