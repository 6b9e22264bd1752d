// cdpr_engine_readout.hip - the read-out: every getter that hands robot-major arrays out (cdpr_get_*), the decoders of a recorded
// observable image and cdpr_set_platform_state*, all on the column table of cdpr_readout.hpp.  One gather kernel (a template over the
// layout's element type, emitted here only), one host routine (read_blocks).  Reference paths as in cdpr_engine.hip.
#include "cdpr_engine_internal.hpp"

namespace cdpr {

// One thread per OUTPUT element, so that a wave writes 256 contiguous bytes (the destination may be host memory behind PCIe).  With a
// completion word: the last workgroup stores the epoch after a system-scope fence and the host spins on that word - no copy engine, no
// runtime call in the wait.
template <typename T>
__global__ __launch_bounds__(256) void cdpr_unpack_publish_kernel(const ReadoutArgs a) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o < a.total) {
    uint32_t off = 0, width = a.width[0], col0 = a.col0[0], k = 0;
#pragma unroll
    for (uint32_t i = 1; i < kReadMaxBlocks; ++i)
      if (i < a.nblocks && o >= a.off[i - 1]) off = a.off[i - 1], width = a.width[i], col0 = a.col0[i], k = i;
    const uint32_t rem = o - off, r = rem / width;
    const T v = static_cast<const T*>(a.rows)[read_element<T>(a.code[col0 + (rem - r * width)], a.stride, r)];
    if ((a.as_int >> k) & 1u)
      static_cast<int32_t*>(a.out)[o] = (int32_t)v;
    else if (a.out_double)
      static_cast<double*>(a.out)[o] = (double)v;
    else
      static_cast<float*>(a.out)[o] = (float)v;
  }
  if (!a.done) return;  // staged read-out: the copy engine and the stream wait finish the job
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = atomicAdd(a.arrivals, 1u);
    if (prev == gridDim.x - 1u) {
      *a.arrivals = 0u;
      __threadfence_system();
      __hip_atomic_store(a.done, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace cdpr

namespace cdpr_host {

static BlockColumns columns_of(const cdpr_engine* h, int block) { return h->plan.fp64 ? row_columns(block, h->n) : slot_columns(block, h->n, h->plan.fk); }

// Where the gathered bytes go, by their number - one record per precision, each as measured for it (not unified: nobody has measured
// the fp64 rule against the fp32 one).  Up to `direct`: the kernel stores into the mapped pinned image (small images: a per-step caller
// of a few robots, ~5 us; kernel stores over PCIe reach ~7 GB/s, the copy engine ~30) and the host waits for the completion word
// (`word`) or the stream.  Up to `staged`, from `staged_blocks` blocks on: device scratch, ONE copy into the pinned image, split up on the host
// (it merges the blocks' copies; one block alone has nothing to merge and the detour would only add the host's copy out of the image).  Beyond:
// device scratch and one copy per block straight into the caller's arrays (reading a large pinned image back costs more than the DMA).
struct ReadTiers { size_t direct; bool word; size_t staged; uint32_t staged_blocks; };
constexpr ReadTiers kTiers32{256u << 10, true, 2u << 20, 2}, kTiers64{2u << 20, false, 0, 0};
constexpr size_t kImageMax = 2u << 20;  // the largest image either record asks for

enum ReadOut { kOutFloat, kOutDouble };
constexpr int kAsInt = 0x100;  // or-ed to a block: it leaves as int32

// wait on the completion word: plain host memory, no runtime call; past the spin budget fall back to the stream wait (which also
// surfaces a device fault instead of spinning on a word that will never come)
static int await_word(cdpr_engine* h, uint64_t epoch) {
  volatile uint64_t* done = h->h_pub_done;
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  while (*done != epoch) {
    if ((++spins & 0x3FFu) == 0 && std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() >= 20) {
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      if (*done != epoch) {
        h->err = "cdpr_get_observables: the publish kernel finished without its completion word";
        return CDPR_ERR_DEVICE;
      }
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return CDPR_OK;
}

// The blocks of ONE source buffer (dst[k] non-null) in one launch and one wait.
static int read_source(cdpr_engine* h, const void* rows, const BlockColumns* cols, void* const* dst, const bool* as_int, int count, ReadOut out) {
  const size_t esz = out == kOutDouble ? sizeof(double) : sizeof(float);
  ReadoutArgs u{};
  size_t total = 0;
  uint32_t ncol = 0;
  void* want[kReadMaxBlocks];
  size_t off[kReadMaxBlocks];  // element offset of a block in `out`
  for (int k = 0; k < count; ++k) {
    if (ncol + cols[k].width > kReadMaxColumns || (as_int[k] && out == kOutDouble)) {
      h->err = "read_blocks: more columns than the gather's table holds, or an integer block among doubles";
      return CDPR_ERR_INVALID;
    }
    const uint32_t b = u.nblocks++;
    u.width[b] = (uint8_t)cols[k].width, u.col0[b] = (uint8_t)ncol, off[b] = total;
    if (b) u.off[b - 1] = (uint32_t)total;  // (below 2^32: checked behind the loop, in front of the launch)
    if (as_int[k]) u.as_int |= (uint8_t)(1u << b);
    memcpy(&u.code[ncol], cols[k].code, cols[k].width * sizeof(uint16_t));
    want[b] = dst[k];
    ncol += cols[k].width;
    total += (size_t)h->batch * cols[k].width;
  }
  if (total >= (1ull << 32)) {  // element offsets are 32-bit: one block at a time
    if (count == 1) {
      h->err = "read_blocks: one array of 2^32 elements or more";
      return CDPR_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < count; ++k)
      if (int rc = read_source(h, rows, cols + k, dst + k, as_int + k, 1, out)) return rc;
    return CDPR_OK;
  }
  const ReadTiers& tier = h->plan.fp64 ? kTiers64 : kTiers32;
  const size_t bytes = total * esz;
  const bool direct = bytes <= tier.direct, staged = !direct && bytes <= tier.staged && u.nblocks >= tier.staged_blocks;
  // lazy set-up, every allocation guarded on its own pointer (a failure half way leaves nothing to leak or to skip next time).
  // Coherent host memory: the host may spin on the completion word while the kernel is still running.
  if ((direct || staged) && !h->h_pub)
    HIP_TRY(h, h->h_pub.alloc(std::min(kImageMax, (size_t)h->batch * kReadMaxColumns * sizeof(double)), hipHostMallocMapped | hipHostMallocCoherent));
  if (direct && tier.word) {
    if (!h->h_pub_done) {
      HIP_TRY(h, h->h_pub_done.alloc(sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));
      *h->h_pub_done = 0;
    }
    if (!h->d_pub_arrivals) {
      HIP_TRY(h, h->d_pub_arrivals.alloc(sizeof(uint32_t)));
      hipError_t me = hipMemsetAsync(h->d_pub_arrivals, 0, sizeof(uint32_t), h->stream);
      if (me != hipSuccess) {  // never launch the gather on an uninitialised arrival counter
        h->d_pub_arrivals.release();
        HIP_TRY(h, me);
      }
    }
    HIP_TRY(h, hipHostGetDevicePointer((void**)&u.done, h->h_pub_done, 0));
    u.arrivals = h->d_pub_arrivals;
    u.epoch = ++h->pub_epoch;
  }
  if (direct) {
    HIP_TRY(h, hipHostGetDevicePointer(&u.out, h->h_pub, 0));
  } else {
    HIP_TRY(h, h->d_unpack.ensure(h, bytes));
    u.out = h->d_unpack;
  }
  u.rows = rows;
  u.stride = h->stride, u.total = (uint32_t)total;
  u.out_double = out == kOutDouble ? 1 : 0;
  const dim3 grid((uint32_t)((total + 255) / 256)), block(256);
  if (h->plan.fp64)
    hipLaunchKernelGGL(cdpr_unpack_publish_kernel<double>, grid, block, 0, h->stream, u);
  else
    hipLaunchKernelGGL(cdpr_unpack_publish_kernel<float>, grid, block, 0, h->stream, u);
  HIP_TRY(h, hipGetLastError());
  if (direct && tier.word) {
    if (int rc = await_word(h, u.epoch)) return rc;
  } else {
    if (staged) HIP_TRY(h, hipMemcpyAsync(h->h_pub, h->d_unpack, bytes, hipMemcpyDeviceToHost, h->stream));
    if (!direct && !staged)
      for (uint32_t b = 0; b < u.nblocks; ++b)
        HIP_TRY(h, hipMemcpyAsync(want[b], h->d_unpack + off[b] * esz, (size_t)h->batch * u.width[b] * esz, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, wait_stream(h));  // (the scratch is reused by the next call)
  }
  if (direct || staged)
    for (uint32_t b = 0; b < u.nblocks; ++b) memcpy(want[b], h->h_pub + off[b] * esz, (size_t)h->batch * u.width[b] * esz);
  return CDPR_OK;
}

// blocks[k] (a ReadBlock, | kAsInt) of every robot into dst[k], a robot-major host array of `out` (int32 for kAsInt); a null dst[k]
// is skipped.  One launch and one wait per source buffer the list touches: the observable image, then the state.
static int read_blocks(cdpr_engine* h, std::initializer_list<int> blocks, std::initializer_list<void*> dst, ReadOut out) {
  for (const bool state : {false, true}) {
    BlockColumns cols[kReadMaxBlocks];
    void* to[kReadMaxBlocks];
    bool as_int[kReadMaxBlocks];
    int count = 0;
    auto d = dst.begin();
    for (const int b : blocks) {
      const BlockColumns c = columns_of(h, b & ~kAsInt);
      void* const to_k = *d++;
      if (!to_k || c.state != state) continue;
      if (count == (int)kReadMaxBlocks) {
        h->err = "read_blocks: more blocks than one gather takes";
        return CDPR_ERR_INVALID;
      }
      cols[count] = c, to[count] = to_k, as_int[count] = (b & kAsInt) != 0, ++count;
    }
    const void* rows = h->plan.fp64 ? (state ? (const void*)h->d_state64.p : h->d_obs64.p) : (state ? (const void*)h->d_state.p : h->d_obs.p);
    if (count)
      if (int rc = read_source(h, rows, cols, to, as_int, count, out)) return rc;
  }
  return CDPR_OK;
}

// A recorded image (layout type T) -> the five robot-major arrays of the published step, as O
template <typename T, typename O>
static void decode_image(const cdpr_engine* h, const void* image, std::initializer_list<O*> dst) {
  int block = kReadPosition;
  for (O* out : dst) {
    const BlockColumns c = columns_of(h, block++);
    if (!out) continue;
    for (uint32_t r = 0; r < h->batch; ++r)
      for (uint32_t j = 0; j < c.width; ++j) out[(size_t)r * c.width + j] = (O)static_cast<const T*>(image)[read_element<T>(c.code[j], h->stride, r)];
  }
}

// Spawn poses and twists (S) into the platform rows of the state (layout type T): fetch the rows, write the columns, upload.
template <typename T, typename S>
static int set_platform(cdpr_engine* h, const S* pose7, const S* twist6) {
  const size_t count = h->plan.fp64 ? (size_t)kF64StateCtrl * h->stride : (size_t)plat_slots(h->plan.fk) * h->stride * 4u;
  void* const d_rows = h->plan.fp64 ? (void*)h->d_state64.p : (void*)h->d_state.p;
  std::vector<T> s(count);
  HIP_TRY(h, hipMemcpyAsync(s.data(), d_rows, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, wait_stream(h));
  const auto put = [&](int block, const S* src, uint32_t src_width) {
    const BlockColumns c = columns_of(h, block);
    for (uint32_t r = 0; r < h->batch; ++r)
      for (uint32_t j = 0; j < c.width; ++j) s[read_element<T>(c.code[j], h->stride, r)] = (T)src[(size_t)r * src_width + j];
  };
  if (pose7) put(kReadRawPose, pose7, 7), put(kReadFkPose, pose7, 7);  // the FK seed follows the spawn pose
  if (twist6) put(kReadRawTwist, twist6, 6);
  HIP_TRY(h, hipMemcpyAsync(d_rows, s.data(), count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, wait_stream(h));
  return CDPR_OK;
}

static int need_fp64(cdpr_engine* h, const char* what) {
  if (h->plan.fp64) return CDPR_OK;
  h->err = std::string(what) + ": the handle was not created with precision = 64";
  return CDPR_ERR_UNSUPPORTED;
}

static int need_stage(cdpr_engine* h, bool on, const char* stage) {
  if (on) return CDPR_OK;
  h->err = std::string(stage) + " not enabled";
  return CDPR_ERR_UNSUPPORTED;
}

}  // namespace cdpr_host

extern "C" {

int cdpr_set_platform_state(cdpr_handle_t h, const float* pose7, const float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return h->plan.fp64 ? set_platform<double>(h, pose7, twist6) : set_platform<float>(h, pose7, twist6);
}

int cdpr_set_platform_state_f64(cdpr_handle_t h, const double* pose7, const double* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = need_fp64(h, "cdpr_set_platform_state_f64")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return set_platform<double>(h, pose7, twist6);
}

int cdpr_decode_observables(cdpr_handle_t h, const void* image, float* position, float* velocity, float* effort, float* pose7, float* twist6) {
  if (!h || !image) return CDPR_ERR_INVALID;
  if (h->plan.fp64)  // (the float getters of a precision = 64 handle round)
    decode_image<double, float>(h, image, {position, velocity, effort, pose7, twist6});
  else
    decode_image<float, float>(h, image, {position, velocity, effort, pose7, twist6});
  return CDPR_OK;
}

int cdpr_decode_observables_f64(cdpr_handle_t h, const void* image, double* position, double* velocity, double* effort, double* pose7, double* twist6) {
  if (!h || !image) return CDPR_ERR_INVALID;
  if (int rc = need_fp64(h, "cdpr_decode_observables_f64")) return rc;
  decode_image<double, double>(h, image, {position, velocity, effort, pose7, twist6});
  return CDPR_OK;
}

int cdpr_get_joint_states(cdpr_handle_t h, float* position, float* velocity, float* effort) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadPosition, kReadVelocity, kReadEffort}, {position, velocity, effort}, kOutFloat));
}

// JointState + PlatformState of the last published step in ONE device round trip (PLG.cpp:248-280 publishes both every step)
int cdpr_get_observables(cdpr_handle_t h, float* position, float* velocity, float* effort, float* pose7, float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadPosition, kReadVelocity, kReadEffort, kReadPose, kReadTwist}, {position, velocity, effort, pose7, twist6}, kOutFloat));
}

int cdpr_get_observables_f64(cdpr_handle_t h, double* position, double* velocity, double* effort, double* pose7, double* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = need_fp64(h, "cdpr_get_observables_f64")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadPosition, kReadVelocity, kReadEffort, kReadPose, kReadTwist}, {position, velocity, effort, pose7, twist6}, kOutDouble));
}

int cdpr_get_platform_state(cdpr_handle_t h, float* pose7, float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadPose, kReadTwist}, {pose7, twist6}, kOutFloat));
}

int cdpr_get_raw_state(cdpr_handle_t h, float* pose7, float* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadRawPose, kReadRawTwist}, {pose7, twist6}, kOutFloat));
}

int cdpr_get_raw_state_f64(cdpr_handle_t h, double* pose7, double* twist6) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = need_fp64(h, "cdpr_get_raw_state_f64")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadRawPose, kReadRawTwist}, {pose7, twist6}, kOutDouble));
}

int cdpr_get_pid_debug(cdpr_handle_t h, float* axes9) {
  if (!h || !axes9) return CDPR_ERR_INVALID;
  if (int rc = need_stage(h, h->dbg, "CDPR_STAGE_PID_DEBUG")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  if (h->plan.fp64) {
    std::vector<double> d((size_t)h->batch * CDPR_PID_DEBUG_AXES);
    HIP_TRY(h, hipMemcpyAsync(d.data(), h->d_dbg64, d.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, wait_stream(h));
    for (size_t i = 0; i < d.size(); ++i) axes9[i] = (float)d[i];
  } else {
    HIP_TRY(h, hipMemcpyAsync(axes9, h->d_dbg, (size_t)h->batch * CDPR_PID_DEBUG_AXES * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, wait_stream(h));
  }
  return checked(h, CDPR_OK);
}

int cdpr_get_fk_state(cdpr_handle_t h, float* pose7, float* residual, int32_t* iterations) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = need_stage(h, h->plan.fk, "CDPR_STAGE_FK")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  return checked(h, read_blocks(h, {kReadFkPose, kReadFkResidual, kReadFkIterations | kAsInt}, {pose7, residual, iterations}, kOutFloat));
}

int cdpr_get_td_state(cdpr_handle_t h, float* tension, int32_t* infeasible) {
  if (!h) return CDPR_ERR_INVALID;
  if (int rc = need_stage(h, h->plan.td, "CDPR_STAGE_TD")) return rc;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  const int rc = read_blocks(h, {kReadEffort, kReadFlags | kAsInt}, {tension, infeasible}, kOutFloat);  // applied force == distributed tension
  if (rc == CDPR_OK && infeasible)
    for (uint32_t b = 0; b < h->batch; ++b) infeasible[b] &= 1;  // the travel-limit mask shares the word (pack_flags)
  return checked(h, rc);
}

int cdpr_get_limit_state(cdpr_handle_t h, uint32_t* cable_mask) {
  if (!h || !cable_mask) return CDPR_ERR_INVALID;
  if (set_device(h) != CDPR_OK) return CDPR_ERR_DEVICE;
  const int rc = read_blocks(h, {kReadFlags | kAsInt}, {cable_mask}, kOutFloat);
  if (rc == CDPR_OK)
    for (uint32_t b = 0; b < h->batch; ++b) cable_mask[b] >>= 1;  // bit 0 is the tension-distribution flag
  return checked(h, rc);
}

}  // extern "C"
