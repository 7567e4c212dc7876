// Who owns a hipMalloc: a DevicePool.  It is a list of the pointers it allocated, nothing more -- no caching, no
// sub-allocation; every alloc() is one hipMalloc of the size asked for.  A long-lived state (rbpf_ctx, SmootherState,
// ShardState, LocState) has one as a member, a function that needs scratch declares one on its stack and returns freely.
#pragma once
#include "../../include/rbpf.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace rbpf {

int hip_fail(hipError_t e, const char* what, const char* file, int line);   // the single error mapping (rbpf_api.hip)

// bytes owned by all pools of this process (rbpf_device_bytes_live): back to its old value once a session is gone
inline std::atomic<long long> g_device_bytes_live{0};

class DevicePool {
 public:
  DevicePool() = default;
  DevicePool(const DevicePool&) = delete;
  DevicePool& operator=(const DevicePool&) = delete;
  ~DevicePool() { clear(); }

  // RBPF_OK, or hip_fail()'s status (out of memory: RBPF_ERR_OUT_OF_MEMORY).  count == 0: *p = nullptr, no call.
  template <typename T>
  int alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) return RBPF_OK;
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    blocks_.emplace_back(q, bytes);
    g_device_bytes_live += (long long)bytes;
    *p = static_cast<T*>(q);
    return RBPF_OK;
  }
  // alloc + blocking copy from the host
  template <typename T>
  int upload(T** p, const T* src, size_t count) {
    const int s = alloc(p, count);
    if (s != RBPF_OK || count == 0) return s;
    const hipError_t e = hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return RBPF_OK;
  }
  // free one buffer early (grow / re-allocate sites); null or a pointer of somebody else: nothing happens
  void release(void* p) {
    for (size_t i = 0; p && i < blocks_.size(); ++i)
      if (blocks_[i].first == p) {
        drop(blocks_[i]);
        blocks_.erase(blocks_.begin() + (std::ptrdiff_t)i);
        return;
      }
  }
  void clear() {
    for (auto& b : blocks_) drop(b);
    blocks_.clear();
  }

 private:
  static void drop(const std::pair<void*, size_t>& b) {
    (void)hipFree(b.first);
    g_device_bytes_live -= (long long)b.second;
  }
  std::vector<std::pair<void*, size_t>> blocks_;
};

}  // namespace rbpf
