// kh_devbuf.h — Dev<T>, a device buffer from the pool that lives as long as the call, and Up, the upload into one.
#ifndef KH_DEVBUF_H_
#define KH_DEVBUF_H_

#include <vector>

#include "kh_common.h"

#pragma GCC visibility push(hidden)   // helpers of the including file, not exports of the library
namespace kh {

// A pool allocation that lives as long as the call.
template <typename T>
struct Dev {
  T *p = nullptr;
  size_t n = 0;   // elements allocated
  Dev() = default;
  Dev(const Dev &) = delete;
  Dev &operator=(const Dev &) = delete;
  ~Dev() { if (p) PoolFree(p); }
  int Alloc(size_t count) {
    if (p) PoolFree(p);
    n = count ? count : 1;
    p = static_cast<T *>(PoolMalloc(sizeof(T) * n));
    return p ? KH_OK : KH_ENOMEM;
  }
  int Grow(size_t count) { return p && count <= n ? KH_OK : Alloc(count); }
  int Upload(const T *h, size_t count, hipStream_t st) {
    if (Alloc(count)) return KH_ENOMEM;
    if (count) KH_HIP(hipMemcpyAsync(p, h, sizeof(T) * count, hipMemcpyHostToDevice, st));
    return KH_OK;
  }
  int Upload(const std::vector<T> &h, hipStream_t st) { return Upload(h.data(), h.size(), st); }
};

// host -> device into a buffer that is already allocated; nothing to do for count == 0
template <typename T>
hipError_t Up(Dev<T> &dev, const T *host, size_t count, hipStream_t st) {
  return count ? hipMemcpyAsync(dev.p, host, sizeof(T) * count, hipMemcpyHostToDevice, st) : hipSuccess;
}

}  // namespace kh
#pragma GCC visibility pop

#endif  // KH_DEVBUF_H_
