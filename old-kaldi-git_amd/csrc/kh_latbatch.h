// kh_latbatch.h — the host scaffolding the batched entry points share (kh_latbest, kh_latprune, kh_latoracle, kh_latmbr,
// kh_latrescore, kh_latalign, kh_align): device buffers (kh_devbuf.h), the events behind last_timings, the
// per-thread call record with its workspace limit, and WaveFence, the one device helper.  Small functions, no framework: a
// new batched lattice entry point starts from these and from kh_latbatch_host.h (validation, incoming lists, chunk plan).
#ifndef KH_LATBATCH_H_
#define KH_LATBATCH_H_

#include <chrono>

#include "kh_common.h"
#include "kh_devbuf.h"
#include "kh_latbatch_host.h"

#pragma GCC visibility push(hidden)   // helpers of the including file, not exports of the library
namespace kh {

// The clock and the four events behind the five slots every *_last_timings reports:
//   0 host_prep  construction .. HostDone()          2 kernel    3 download   (events; Add() sums them over the launches)
//   1 upload                                          4 call      construction .. Finish()
struct CallTimer {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t1 = t0;
  float up = 0.f, kernel = 0.f, down = 0.f;
  CallTimer() = default;
  CallTimer(const CallTimer &) = delete;
  CallTimer &operator=(const CallTimer &) = delete;
  ~CallTimer() { for (int i = 0; i < 4; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); }
  static float Ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<float, std::milli>(b - a).count();
  }
  void HostDone() { t1 = std::chrono::steady_clock::now(); }
  hipError_t Init() {
    for (int i = 0; i < 4; i++) {
      const hipError_t e = hipEventCreate(&ev[i]);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  hipError_t Mark(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
  // *acc += the time between two marks the stream has passed
  hipError_t Add(float *acc, int from, int to) {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, ev[from], ev[to]);
    *acc += ms;
    return e;
  }
  // marks 0..3 taken once around upload, kernels and download
  hipError_t AddAll() {
    hipError_t e = Add(&up, 0, 1);
    if (e == hipSuccess) e = Add(&kernel, 1, 2);
    if (e == hipSuccess) e = Add(&down, 2, 3);
    return e;
  }
  void Finish(float *ms5) const {
    ms5[0] = Ms(t0, t1);
    ms5[1] = up;
    ms5[2] = kernel;
    ms5[3] = down;
    ms5[4] = Ms(t0, std::chrono::steady_clock::now());
  }
};

// What an entry point remembers of the calling thread's last call; every .hip keeps a thread_local one of its own, so the
// workspace limit stays per entry point and per thread.
template <int NMs, int NCounts>
struct CallStats {
  float ms[NMs] = {};
  int32_t counts[NCounts] = {};
  size_t workspace_limit = 0;   // 0: DefaultWorkspaceLimit
};

template <int NMs, int NCounts>
int GetTimings(const CallStats<NMs, NCounts> &stats, float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms);
  for (int i = 0; i < NMs; i++) ms[i] = stats.ms[i];
  if (counts) for (int i = 0; i < NCounts; i++) counts[i] = stats.counts[i];
  return KH_OK;
}

// Half of what is left of the device's memory (the pool's cached blocks count as free) after the buffers whose size the
// input fixes; a quarter of it when those take more than half.
inline int DefaultWorkspaceLimit(size_t fixed_bytes, size_t *limit) {
  size_t free_b = 0, total_b = 0;
  const int rc = kh_mem_info(&free_b, &total_b);
  if (rc != KH_OK) return rc;
  const size_t avail = free_b + PoolCachedBytes();
  *limit = avail > 2 * fixed_bytes ? (avail - fixed_bytes) / 2 : avail / 4;
  return KH_OK;
}

// memory written by some lanes and read by others of the same wave later in program order
__device__ __forceinline__ void WaveFence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace kh
#pragma GCC visibility pop

#endif  // KH_LATBATCH_H_
