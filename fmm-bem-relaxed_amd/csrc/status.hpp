// status.hpp -- the helpers shared by the host code behind the C ABI (plan.hip, ops.hip, direct.hip, krylov.hip): how it reports
// a failure, pins a call to its device and holds a call's device memory.  Includes no HIP header: it comes after <hip/hip_runtime.h> and include/fmmbem.h in a file that uses it.
#pragma once
#include <string>
#include <vector>

namespace fmmbem {
int fail(int code, const std::string& msg);           // plan.hip: records the message for fmmbem_last_error
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return ::fmmbem::fail(e_ == hipErrorOutOfMemory ? FMMBEM_ERR_ALLOC : FMMBEM_ERR_HIP,        \
                            std::string(#expr) + ": " + hipGetErrorString(e_));                    \
  } while (0)
#define TRY(expr) do { int rc_ = (expr); if (rc_ != FMMBEM_OK) return rc_; } while (0)

namespace fmmbem {

// The C ABI takes a device ordinal per plan; every entry point that touches the device switches to it and restores the
// caller's current device on the way out (a process may hold plans on several devices, and torch keeps its own idea of
// the current device).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err != hipSuccess) { prev = -1; return; }
    if (prev != dev) err = hipSetDevice(dev); else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// device memory of one call (ops.hip, direct.hip), freed when the call returns
struct Scratch {
  std::vector<void*> v;
  ~Scratch() { for (void* p : v) (void)hipFree(p); }
  template <class T>
  int alloc(size_t count, T** dst) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, count ? count * sizeof(T) : 1));
    v.push_back(p);
    *dst = static_cast<T*>(p);
    return FMMBEM_OK;
  }
  template <class T>
  int up(const T* src, size_t count, const T** dst) {
    T* p = nullptr;
    TRY(alloc(count, &p));
    if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = p;
    return FMMBEM_OK;
  }
  template <class T>
  int zeros(size_t count, T** dst, hipStream_t s) {
    T* p = nullptr;
    TRY(alloc(count, &p));
    if (count) HIP_TRY(hipMemsetAsync(p, 0, count * sizeof(T), s));
    *dst = p;
    return FMMBEM_OK;
  }
};

}  // namespace fmmbem
