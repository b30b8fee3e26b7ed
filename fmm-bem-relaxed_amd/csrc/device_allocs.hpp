// device_allocs.hpp -- the device memory a handle owns (fmmbem_plan: two of these, the shared geometry's and the plan's own;
// fmmbem_ops; fmmbem_direct): every allocation is recorded and freed with its owner.  Comes after <hip/hip_runtime.h> and
// include/fmmbem.h, like status.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "device_plan.hpp"
#include "shift_ops.hpp"
#include "status.hpp"

namespace fmmbem {

struct DeviceAllocs {
  std::vector<void*> list;
  int device = 0;                                      // where the list lives: the destructor frees it there
  DeviceAllocs() = default;
  DeviceAllocs(const DeviceAllocs&) = delete;
  DeviceAllocs& operator=(const DeviceAllocs&) = delete;
  ~DeviceAllocs() {
    if (list.empty()) return;
    DeviceGuard guard(device);
    free_all();
  }
  void free_all() {                                    // on the current device
    for (void* p : list) (void)hipFree(p);
    list.clear();
  }
  void free_one(const void* p) {                       // creation-time scratch
    (void)hipFree(const_cast<void*>(p));
    list.erase(std::find(list.begin(), list.end(), p));
  }
  template <class T>
  int alloc(size_t count, T** out, bool zero) {        // (the zero-fill runs on the NULL stream)
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIP_TRY(hipMalloc(&p, bytes));
    list.push_back(p);
    if (zero) HIP_TRY(hipMemset(p, 0, bytes));
    *out = static_cast<T*>(p);
    return FMMBEM_OK;
  }
  template <class T>
  int upload(const T* src, size_t count, const T** out) {
    *out = nullptr;
    T* p = nullptr;
    TRY(alloc(count, &p, false));
    if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return FMMBEM_OK;
  }
  template <class T, class A>
  int upload(const std::vector<T, A>& v, const T** out) { return upload(v.data(), v.size(), out); }
};

// the sparse shift operators of every order up to ops.P, index p - 1
inline int upload_shift_ops(DeviceAllocs& mem, const ShiftOps& ops, std::vector<ShiftOpDev>& up, std::vector<ShiftOpDev>& down) {
  auto one = [&](const VOp& v, ShiftOpDev& o) -> int {
    TRY(mem.upload(v.src, &o.src)); TRY(mem.upload(v.y, &o.y)); TRY(mem.upload(v.real, &o.real));
    TRY(mem.upload(v.npiece, &o.npiece)); TRY(mem.upload(v.piece, &o.piece));
    o.T = v.T; o.V = v.V; o.maxp = v.maxp;
    return FMMBEM_OK;
  };
  up.resize(ops.P); down.resize(ops.P);
  for (int p = 1; p <= ops.P; ++p) { TRY(one(ops.up_v[p - 1], up[p - 1])); TRY(one(ops.down_v[p - 1], down[p - 1])); }
  return FMMBEM_OK;
}

}  // namespace fmmbem
