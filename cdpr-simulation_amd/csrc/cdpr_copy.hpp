// cdpr_copy.hpp — fork robots of a per-robot handle (cdpr_copy_robots[_device]): robot r with 0 <= source[r] < B, source[r] != r takes
// over, to the bit, everything robot-indexed the handle owns of robot s = source[r]; every other robot is neither read (but as a
// source) nor written.  A source is itself untouched (source[s] < 0 or source[s] == s), so sources are only read and destinations only
// written: one launch, no scratch copy, no hazard.  The world step is the same for both, so nothing is rebased - the rings that follow
// the world step, the stamps and the `step + 1` hot word are bits moved.  One kernel per record layout, as cdpr_reset.hpp.
//
// One thread per destination index, 256 per block, the map entry read once, a non-destination leaves at once.  Every store is
// row * stride + r (neighbouring destinations coalesce), every load row * stride + s.  The loads of a column go out kCopyBatch at a
// time in front of their stores: a lone destination in its wave pays one round trip per batch, not one per row.  No LDS, no scratch.
#pragma once
#include "../../include/cdpr.h"
#include "cdpr_kernels.hpp"

namespace cdpr {

constexpr int kCopyBatch = 8;  // independent loads in flight per destination
// a float4 slot as the bits it holds (packed words included): a native vector, which a batch keeps in registers
using CopySlot = uint32_t __attribute__((ext_vector_type(4)));

// what the three kernels share: who takes whom, and the counts
struct CopyWho {
  const int32_t* source;    // int32[B]
  uint32_t* status;         // uint32[2] = [copied, skipped], zeroed on the stream in front of the launch; or nullptr
  uint32_t* episode_start;  // uint32[B] (cdpr_get_episode_start)
  uint32_t batch;
};

// The thread's verdict: true for a destination with a valid source `s`.  A destination whose source is out of range or is itself a
// destination is skipped and counted in status[1].  Every lane of the wave comes through here (one ballot + popcount per count, an
// ordinary atomicAdd by lane 0, as done_store has it).
CDPR_DEV bool copy_verdict(const CopyWho& w, uint32_t r, uint32_t& s) {
  const int32_t v = r < w.batch ? w.source[r] : -1;
  const bool wants = v >= 0 && (uint32_t)v != r;
  bool ok = wants && (uint32_t)v < w.batch;
  if (ok) {
    const int32_t up = w.source[v];
    ok = up < 0 || up == v;
  }
  s = ok ? (uint32_t)v : r;
  if (w.status) {  // (wave-uniform)
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    const uint32_t copied = (uint32_t)__popcll(__ballot(ok)), skipped = (uint32_t)__popcll(__ballot(wants && !ok));
    if (lane0 && copied) atomicAdd(w.status, copied);
    if (lane0 && skipped) atomicAdd(w.status + 1, skipped);
  }
  return ok;
}

// rows [0, rows) of a column-per-robot buffer: base[row * stride + r] = base[row * stride + s]
template <typename T>
CDPR_DEV void copy_column(T* base, size_t stride, uint32_t rows, uint32_t r, uint32_t s) {
  const T* const src = base + s;
  T* const dst = base + r;
  uint32_t row = 0;
  for (; row + kCopyBatch <= rows; row += kCopyBatch) {
    T v[kCopyBatch];
#pragma unroll
    for (int j = 0; j < kCopyBatch; ++j) v[j] = src[(size_t)(row + j) * stride];
#pragma unroll
    for (int j = 0; j < kCopyBatch; ++j) dst[(size_t)(row + j) * stride] = v[j];
  }
  for (; row < rows; ++row) dst[(size_t)row * stride] = src[(size_t)row * stride];
}

// a robot-major row: base[r * width + c] = base[s * width + c] (the active target, the latched commands, the `pid` debug row)
template <typename T>
CDPR_DEV void copy_row(T* base, uint32_t width, uint32_t r, uint32_t s) {
  if (!base) return;
  for (uint32_t c = 0; c < width; ++c) base[(size_t)r * width + c] = base[(size_t)s * width + c];
}

// Register-resident per-robot records: every state slot row (platform, FK estimate, ring rows, integral rows), the observable image,
// the `pid` row, meta (mode and Pid call count), the active target row, the episode-clock word.
struct CopyFastArgs {
  CopyWho who;
  float4* state;
  float4* obs;
  float* dbg;           // float[B][9], or nullptr
  uint8_t* meta;        // StepArgs::meta
  float* target;        // float[B][n]
  size_t stride;
  uint32_t n_state, n_obs, n;
};

static __global__ __launch_bounds__(256) void cdpr_copy_fast_kernel(const CopyFastArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t s;
  if (!copy_verdict(a.who, r, s)) return;
  copy_column(reinterpret_cast<CopySlot*>(a.state), a.stride, a.n_state, r, s);
  copy_column(reinterpret_cast<CopySlot*>(a.obs), a.stride, a.n_obs, r, s);
  copy_row(a.dbg, CDPR_PID_DEBUG_AXES, r, s);
  a.meta[r] = a.meta[s];
  copy_row(a.target, a.n, r, s);
  a.who.episode_start[r] = a.who.episode_start[s];
}

// General path: the platform slots and the image; the robot's whole column of the record buffer - region A (float4 slots), region B
// (dword rows) and EVERY region C row: the hot-row word travels with the stale H slots it stands for, so nothing is flushed or
// restored, and its mask and integral words travel too; the mode byte; its rows of the three latched command buffers.
struct CopyGenArgs {
  CopyWho who;
  float4* state;
  float4* obs;
  float* dbg;
  uint8_t* mode;
  float* latched[3];    // float[B][n] per command kind
  float* rec;
  size_t stride;
  uint32_t n_state, n_obs, n;
  GenLayout lay;
};

static __global__ __launch_bounds__(256) void cdpr_copy_gen_kernel(const CopyGenArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t s;
  if (!copy_verdict(a.who, r, s)) return;
  copy_column(reinterpret_cast<CopySlot*>(a.state), a.stride, a.n_state, r, s);
  copy_column(reinterpret_cast<CopySlot*>(a.obs), a.stride, a.n_obs, r, s);
  copy_row(a.dbg, CDPR_PID_DEBUG_AXES, r, s);
  copy_column(reinterpret_cast<CopySlot*>(a.rec), a.stride, (uint32_t)a.lay.slots(), r, s);
  copy_column(a.rec + (size_t)a.lay.slots() * a.stride * 4, a.stride, (uint32_t)(a.lay.rows() + a.lay.hot_rows()), r, s);
  a.mode[r] = a.mode[s];
#pragma unroll
  for (int k = 0; k < 3; ++k) copy_row(a.latched[k], a.n, r, s);
  a.who.episode_start[r] = a.who.episode_start[s];
}

// precision = 64: every double row of the state column at whatever record width the handle has (`state_rows`: plain rings, or the
// HOLD records behind them with their packed words - bits moved, never computed with: the rows go as 64-bit integers), the double
// image and `pid` row, meta, the active target row, the episode word.
struct CopyF64Args {
  CopyWho who;
  double* state;
  double* obs;
  double* dbg;          // double[B][9], or nullptr
  uint8_t* meta;
  float* target;        // float[B][n]
  size_t stride;
  uint32_t state_rows, obs_rows, n;
};

static __global__ __launch_bounds__(256) void cdpr_copy_f64_kernel(const CopyF64Args a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  uint32_t s;
  if (!copy_verdict(a.who, r, s)) return;
  copy_column(reinterpret_cast<uint64_t*>(a.state), a.stride, a.state_rows, r, s);
  copy_column(reinterpret_cast<uint64_t*>(a.obs), a.stride, a.obs_rows, r, s);
  copy_row(reinterpret_cast<uint64_t*>(a.dbg), CDPR_PID_DEBUG_AXES, r, s);
  a.meta[r] = a.meta[s];
  copy_row(a.target, a.n, r, s);
  a.who.episode_start[r] = a.who.episode_start[s];
}

}  // namespace cdpr
