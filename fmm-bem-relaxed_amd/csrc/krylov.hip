// krylov.hip -- the modified Gram-Schmidt column of the callers above the matvec (examples/BEM/GMRES.hpp:203-212,
// GMRES_Stokes.hpp the same loop on Vec<3,double> values): for k = 0..i:  h_k = <w, V_k>;  w -= h_k V_k;  then
// h_{i+1} = |w|,  V_{i+1} = w / h_{i+1}.  The reference runs 2(i + 1) + 2 passes over the vectors; so did solver.py with
// one torch call each, and at N = 1M the 27 iterations of the config-5 solve spent 5-6 ms of 37 there, most of it per-call
// overhead.  Here a column is ONE call and i + 3 launches: launch k subtracts h_{k-1} V_{k-1} and, on the updated w,
// accumulates <w, V_k> in the same sweep (the last launch accumulates <w, w>), then one scales and one collects the column.
// A dot product is 1 024 per-workgroup sums that whoever needs the total adds in index order: same bits every run.
// Same operations in the same order as the reference's loop; only the association inside a dot product differs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fmmbem.h"
#include "status.hpp"
#include "switches.hpp"

namespace fmmbem {
struct SolverWs;
// plan.hip: where a plan lives, how many unknowns it has, and the slot in which it keeps the workspace of the solver below
// (freed with the plan through solver_ws_destroy)
int plan_solver_info(fmmbem_plan* plan, int* device, int64_t* unknowns, int* p_max, SolverWs*** slot);
void solver_ws_destroy(SolverWs* ws);
size_t plan_unknowns(const fmmbem_plan* plan);      // plan.hip: doubles of one x vector (any plan, host-only ones included)
bool plan_block_inverse_built(const fmmbem_plan* plan);   // plan.hip: fmmbem_plan_block_inverse_build has succeeded on it
}

namespace {

constexpr int kBlocks = 1024, kThreads = 256;       // workgroups of a sweep = partial sums per dot product

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of the kBlocks partial sums of one dot product, the same order in every workgroup that asks (unused slots hold zeros)
__device__ __forceinline__ double block_total(const double* __restrict__ partial, double* wsum) {
  double v[kBlocks / kThreads];
#pragma unroll
  for (int u = 0; u < kBlocks / kThreads; ++u) v[u] = partial[threadIdx.x + u * kThreads];
  double s = 0;
#pragma unroll
  for (int u = 0; u < kBlocks / kThreads; ++u) s += v[u];
  s = wave_sum64(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) t += wsum[k];
  return t;
}

// w -= h_prev * v_prev (when v_prev; h_prev = the total of part_prev, formed by every workgroup for itself -- no atomics, no
// device-wide fences: on this part a device-scope fence per workgroup writes the L2 back and cost 30 us per sweep), then this
// workgroup's share of <w, v_dot> (v_dot == nullptr: <w, w>) into part_out[blockIdx.x]
// vec: every vector of the call starts on a 16-byte boundary (the host checks the pointers and the stride); otherwise -- an odd
// ldv with Laplace's one unknown per panel puts every other row of V on an 8-byte boundary -- the whole sweep is scalar
__global__ __launch_bounds__(kThreads) void mgs_step_kernel(int64_t n, double* __restrict__ w, const double* __restrict__ v_prev,
                                                             const double* __restrict__ part_prev, const double* __restrict__ v_dot,
                                                             double* __restrict__ part_out, int vec) {
  __shared__ double wsum[kThreads / 64];
  const double hp = v_prev ? block_total(part_prev, wsum) : 0.0;
  double acc = 0;
  // the slots of this row no workgroup of this grid writes are part of every total: zero them here, every call (a scratch
  // reused after a call with a larger n would otherwise add stale partial sums)
  if (blockIdx.x == 0)
    for (int k = gridDim.x + threadIdx.x; k < kBlocks; k += kThreads) part_out[k] = 0.0;
  // four consecutive elements per thread and step, as two 16-byte vectors per array: all loads of a step are in flight before
  // the first FMA
  const int64_t n4 = vec ? n >> 2 : 0;
  typedef double dv2 __attribute__((ext_vector_type(2)));
  dv2* w2 = reinterpret_cast<dv2*>(w);
  const dv2* p2 = reinterpret_cast<const dv2*>(v_prev);
  const dv2* d2 = reinterpret_cast<const dv2*>(v_dot);
  for (int64_t q = blockIdx.x * (int64_t)kThreads + threadIdx.x; q < n4; q += (int64_t)gridDim.x * kThreads) {
    dv2 wa = w2[2 * q], wb = w2[2 * q + 1];
    dv2 pa = {0, 0}, pb = {0, 0}, da, db;
    if (v_prev) { pa = p2[2 * q]; pb = p2[2 * q + 1]; }
    if (v_dot) { da = d2[2 * q]; db = d2[2 * q + 1]; }
    if (v_prev) {
      wa.x = fma(-hp, pa.x, wa.x); wa.y = fma(-hp, pa.y, wa.y); wb.x = fma(-hp, pb.x, wb.x); wb.y = fma(-hp, pb.y, wb.y);
      w2[2 * q] = wa; w2[2 * q + 1] = wb;
    }
    if (!v_dot) { da = wa; db = wb; }
    acc = fma(wa.x, da.x, acc); acc = fma(wa.y, da.y, acc); acc = fma(wb.x, db.x, acc); acc = fma(wb.y, db.y, acc);
  }
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {   // n mod 4 leftovers
    double wi = w[i];
    if (v_prev) { wi = fma(-hp, v_prev[i], wi); w[i] = wi; }
    acc = fma(wi, v_dot ? v_dot[i] : wi, acc);
  }
  acc = wave_sum64(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int k = 0; k < kThreads / 64; ++k) s += wsum[k];
    part_out[blockIdx.x] = s;
  }
}

// The sweep of mgs_step_kernel on its vector path, statement for statement, as a function: the multi-system kernel below, the
// solver's, runs it once per system (whose vectors always start on 16-byte boundaries).  mgs_step_kernel itself, the kernel of
// fmmbem_mgs_column_device, stays as it is -- wrapping it round this function moves its instructions -- so the two must be
// kept in step ("Multi-right-hand-side GMRES").
__device__ __forceinline__ void mgs_step_body(int64_t n, double* __restrict__ w, const double* __restrict__ v_prev,
                                              const double* __restrict__ part_prev, const double* __restrict__ v_dot,
                                              double* __restrict__ part_out) {
  __shared__ double wsum[kThreads / 64];
  const double hp = v_prev ? block_total(part_prev, wsum) : 0.0;
  double acc = 0;
  // the slots of this row no workgroup of this grid writes are part of every total: zero them here, every call (a scratch
  // reused after a call with a larger n would otherwise add stale partial sums)
  if (blockIdx.x == 0)
    for (int k = gridDim.x + threadIdx.x; k < kBlocks; k += kThreads) part_out[k] = 0.0;
  // four consecutive elements per thread and step, as two 16-byte vectors per array: all loads of a step are in flight before
  // the first FMA
  const int64_t n4 = n >> 2;
  typedef double dv2 __attribute__((ext_vector_type(2)));
  dv2* w2 = reinterpret_cast<dv2*>(w);
  const dv2* p2 = reinterpret_cast<const dv2*>(v_prev);
  const dv2* d2 = reinterpret_cast<const dv2*>(v_dot);
  for (int64_t q = blockIdx.x * (int64_t)kThreads + threadIdx.x; q < n4; q += (int64_t)gridDim.x * kThreads) {
    dv2 wa = w2[2 * q], wb = w2[2 * q + 1];
    dv2 pa = {0, 0}, pb = {0, 0}, da, db;
    if (v_prev) { pa = p2[2 * q]; pb = p2[2 * q + 1]; }
    if (v_dot) { da = d2[2 * q]; db = d2[2 * q + 1]; }
    if (v_prev) {
      wa.x = fma(-hp, pa.x, wa.x); wa.y = fma(-hp, pa.y, wa.y); wb.x = fma(-hp, pb.x, wb.x); wb.y = fma(-hp, pb.y, wb.y);
      w2[2 * q] = wa; w2[2 * q + 1] = wb;
    }
    if (!v_dot) { da = wa; db = wb; }
    acc = fma(wa.x, da.x, acc); acc = fma(wa.y, da.y, acc); acc = fma(wb.x, db.x, acc); acc = fma(wb.y, db.y, acc);
  }
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {   // n mod 4 leftovers
    double wi = w[i];
    if (v_prev) { wi = fma(-hp, v_prev[i], wi); w[i] = wi; }
    acc = fma(wi, v_dot ? v_dot[i] : wi, acc);
  }
  acc = wave_sum64(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int k = 0; k < kThreads / 64; ++k) s += wsum[k];
    part_out[blockIdx.x] = s;
  }
}

// The systems of one launch of the solver below: blockIdx.y picks a workspace slot from a table passed by value
constexpr int kSysPerLaunch = 64;
struct SysTable {
  int count;
  int slot[kSysPerLaunch];
};

// mgs_step_kernel for several systems at once: system blockIdx.y works on its own w, its own column of V and its own rows of
// partial sums, all `slot` strides from the bases; the x dimension, and with it every sum, is the single kernel's
__global__ __launch_bounds__(kThreads) void mgs_step_multi_kernel(int64_t n, double* __restrict__ w, const double* __restrict__ v_prev,
                                                                   const double* __restrict__ part_prev, const double* __restrict__ v_dot,
                                                                   double* __restrict__ part_out, int64_t ld, int64_t part_stride, SysTable t) {
  const int64_t j = t.slot[blockIdx.y];
  mgs_step_body(n, w + j * ld, v_prev ? v_prev + j * ld : nullptr, part_prev ? part_prev + j * part_stride : nullptr,
                v_dot ? v_dot + j * ld : nullptr, part_out + j * part_stride);
}

// x += a z
__global__ __launch_bounds__(kThreads) void mgs_axpy_kernel(int64_t n, double* __restrict__ x, double a, const double* __restrict__ z) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) x[i] = fma(a, z[i], x[i]);
}

// v_next = w / |w|, |w|^2 = the total of part_norm
__global__ __launch_bounds__(kThreads) void mgs_scale_kernel(int64_t n, const double* __restrict__ w, const double* __restrict__ part_norm,
                                                              double* __restrict__ v_next, int vec) {
  __shared__ double wsum[kThreads / 64];
  const double inv = 1.0 / sqrt(block_total(part_norm, wsum));
  typedef double dv2 __attribute__((ext_vector_type(2)));
  const int64_t n2 = vec ? n >> 1 : 0;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n2; q += (int64_t)gridDim.x * blockDim.x) {
    dv2 v = reinterpret_cast<const dv2*>(w)[q];
    v.x *= inv; v.y *= inv;
    reinterpret_cast<dv2*>(v_next)[q] = v;
  }
  for (int64_t i = (n2 << 1) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v_next[i] = w[i] * inv;
}

// mgs_scale_kernel as a function, for the multi-system kernel (see mgs_step_body)
__device__ __forceinline__ void mgs_scale_body(int64_t n, const double* __restrict__ w, const double* __restrict__ part_norm,
                                               double* __restrict__ v_next) {
  __shared__ double wsum[kThreads / 64];
  const double inv = 1.0 / sqrt(block_total(part_norm, wsum));
  typedef double dv2 __attribute__((ext_vector_type(2)));
  const int64_t n2 = n >> 1;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n2; q += (int64_t)gridDim.x * blockDim.x) {
    dv2 v = reinterpret_cast<const dv2*>(w)[q];
    v.x *= inv; v.y *= inv;
    reinterpret_cast<dv2*>(v_next)[q] = v;
  }
  for (int64_t i = (n2 << 1) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v_next[i] = w[i] * inv;
}

__global__ __launch_bounds__(kThreads) void mgs_scale_multi_kernel(int64_t n, const double* __restrict__ w, const double* __restrict__ part_norm,
                                                                    double* __restrict__ v_next, int64_t ld, int64_t part_stride, SysTable t) {
  const int64_t j = t.slot[blockIdx.y];
  mgs_scale_body(n, w + j * ld, part_norm + j * part_stride, v_next + j * ld);
}

// h[k] = total of the k-th row of partial sums, k <= ncols; the last one is |w|^2 -> |w|
__global__ __launch_bounds__(kThreads) void mgs_finish_kernel(const double* __restrict__ partial, int ncols, double* __restrict__ h) {
  __shared__ double wsum[kThreads / 64];
  const double t = block_total(partial + (size_t)blockIdx.x * kBlocks, wsum);
  if (threadIdx.x == 0) h[blockIdx.x] = (int)blockIdx.x == ncols ? sqrt(t) : t;
}

// the same for several systems: the columns land one after the other in launch order (ncols + 1 doubles each), so that all of
// them cross to the host in one copy
__global__ __launch_bounds__(kThreads) void mgs_finish_multi_kernel(const double* __restrict__ partial, int ncols, double* __restrict__ h,
                                                                     int64_t part_stride, SysTable t) {
  __shared__ double wsum[kThreads / 64];
  const double v = block_total(partial + t.slot[blockIdx.y] * part_stride + (size_t)blockIdx.x * kBlocks, wsum);
  if (threadIdx.x == 0) h[(size_t)blockIdx.y * (ncols + 1) + blockIdx.x] = (int)blockIdx.x == ncols ? sqrt(v) : v;
}

}  // namespace

extern "C" int fmmbem_mgs_column_device(int64_t n, double* d_w, const double* d_V, int64_t ldv, int ncols, double* d_h,
                                        double* d_vnext, double* d_scratch, void* stream) {
  if (n <= 0 || !d_w || !d_V || ncols < 1 || !d_h || !d_vnext || !d_scratch || ldv < n)
    return fmmbem::fail(FMMBEM_ERR_INVALID, "fmmbem_mgs_column_device: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t want = (n / 4 + kThreads - 1) / kThreads + 1;
  const int grid = (int)(want < kBlocks ? want : kBlocks);          // slots grid .. kBlocks-1 of a row are zeroed by the sweep itself
  const auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = a16(d_w) && a16(d_V) && a16(d_vnext) && (ldv & 1) == 0;
  for (int k = 0; k <= ncols; ++k) {
    const double* v_prev = k ? d_V + (int64_t)(k - 1) * ldv : nullptr;
    const double* v_dot = k < ncols ? d_V + (int64_t)k * ldv : nullptr;
    hipLaunchKernelGGL(mgs_step_kernel, dim3(grid), dim3(kThreads), 0, s, n, d_w, v_prev, k ? d_scratch + (size_t)(k - 1) * kBlocks : nullptr,
                       v_dot, d_scratch + (size_t)k * kBlocks, vec);
  }
  hipLaunchKernelGGL(mgs_scale_kernel, dim3(grid), dim3(kThreads), 0, s, n, d_w, d_scratch + (size_t)ncols * kBlocks, d_vnext, vec);
  hipLaunchKernelGGL(mgs_finish_kernel, dim3(ncols + 1), dim3(kThreads), 0, s, d_scratch, ncols, d_h);
  return hipGetLastError() == hipSuccess ? FMMBEM_OK : fmmbem::fail(FMMBEM_ERR_HIP, "fmmbem_mgs_column_device: launch failed");
}

extern "C" int fmmbem_mgs_scratch_doubles(int max_cols) { return (max_cols + 1) * kBlocks; }


// ================================================================================================================
// Relaxed GMRES / FGMRES resident on the device (include/fmmbem.h; examples/BEM/GMRES.hpp:143-252, :276-380,
// GMRES_Stokes.hpp:173-320, SolverOptions.hpp:25-38) for k >= 1 right-hand sides on one plan: k independent solves advanced
// in lockstep.  Host side, per system: the (R+1) x R Hessenberg matrix, the Givens rotations, the residual estimate,
// predict_p, back substitution.  Device side: everything of length n.  fmmbem_gmres(_device) is k = 1.
// ================================================================================================================
namespace {

// w += a v, and this workgroup's share of <w, w> afterwards into part_out (r0 = A x0 - b and its norm in one sweep;
// v == nullptr: only the norm)
__global__ __launch_bounds__(kThreads) void axpy_norm_kernel(int64_t n, double* __restrict__ w, double a, const double* __restrict__ v,
                                                              double* __restrict__ part_out) {
  __shared__ double wsum[kThreads / 64];
  if (blockIdx.x == 0)
    for (int k = gridDim.x + threadIdx.x; k < kBlocks; k += kThreads) part_out[k] = 0.0;
  double acc = 0;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    double wi = w[i];
    if (v) { wi = fma(a, v[i], wi); w[i] = wi; }
    acc = fma(wi, wi, acc);
  }
  acc = wave_sum64(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int k = 0; k < kThreads / 64; ++k) s += wsum[k];
    part_out[blockIdx.x] = s;
  }
}

// out = a * in  (V_0 = -w / beta)
__global__ __launch_bounds__(kThreads) void scale_kernel(int64_t n, const double* __restrict__ in, double a, double* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) out[i] = a * in[i];
}

// out = r .* in for every system of the table, `slot` strides of ld from the bases: the diagonal preconditioner in one launch
__global__ __launch_bounds__(kThreads) void scale_multi_kernel(int64_t n, const double* __restrict__ in, const double* __restrict__ r,
                                                                double* __restrict__ out, int64_t ld, SysTable t) {
  const int64_t off = t.slot[blockIdx.y] * ld;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    out[off + i] = r[i] * in[off + i];
}

// x += sum_j y[j] * (r .* B_j), j ascending as the reference's loop (GMRES.hpp:237-241 with M = identity or diagonal;
// FGMRES :368-371 with B = Z): the basis is read once, x once
__global__ __launch_bounds__(kThreads) void update_x_kernel(int64_t n, double* __restrict__ x, const double* __restrict__ B, int64_t ldb, int ncols,
                                                             const double* __restrict__ y, const double* __restrict__ r) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    double acc = x[i];
    const double ri = r ? r[i] : 1.0;
    for (int j = 0; j < ncols; ++j) {
      const double b = B[(int64_t)j * ldb + i];
      acc = fma(y[j], r ? ri * b : b, acc);
    }
    x[i] = acc;
  }
}

}  // namespace

namespace fmmbem {

// Workspace of the solver, kept with the plan between solves: `cap` systems side by side.  Column c of system j is at
// ((c * cap) + j) * ld of V (and Z), w and z of system j at j * ld: column c of all systems is equally spaced, so one batched
// execute takes it as it lies.  A solve of fewer systems than cap runs in the first slots of the wider workspace.
struct SolverWs {
  int device = 0;
  int cap = 0;
  int64_t n = 0, ld = 0;
  int vcols = 0, zcols = 0, hcap = 0;
  double *V = nullptr, *Z = nullptr, *w = nullptr, *z = nullptr, *d_h = nullptr, *d_scratch = nullptr, *d_y = nullptr;
  double *d_xb = nullptr, *d_recip = nullptr;       // staging of the host-pointer entry points
  size_t xb_doubles = 0;
  double* h_pin = nullptr;                          // pinned, 2 * cap * hcap: the Hessenberg columns, then the y coefficients
};

void solver_ws_destroy(SolverWs* ws) {
  if (!ws) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ws->device);
  for (double* p : {ws->V, ws->Z, ws->w, ws->z, ws->d_h, ws->d_scratch, ws->d_y, ws->d_xb, ws->d_recip})
    if (p) (void)hipFree(p);
  if (ws->h_pin) (void)hipHostFree(ws->h_pin);
  (void)hipSetDevice(prev);
  delete ws;
}

}  // namespace fmmbem

namespace {

using fmmbem::SolverWs;
using fmmbem::fail;
using fmmbem::DeviceGuard;

// FMMBEM_KRYLOV_FAIL_GROW=k (tests only): the k-th allocation of the solver workspace in this process fails once, as an
// out-of-memory would -- the retry path of ensure_ws cannot be exercised otherwise without filling 288 GB
int grow(double** p, size_t doubles) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  static int calls = 0;
  const int fail_at = fmmbem::sw::krylov_fail_grow();
  if (fail_at > 0 && ++calls == fail_at) return fail(FMMBEM_ERR_ALLOC, "solver workspace: allocation failure injected by FMMBEM_KRYLOV_FAIL_GROW");
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), sizeof(double) * std::max<size_t>(doubles, 1)));
  return FMMBEM_OK;
}

// after a failed allocation: nothing of the workspace is trusted -- every buffer freed, every size zero, so that the next solve
// on this plan allocates from scratch instead of launching on the null pointers a half-grown workspace holds
void reset_ws(SolverWs* ws) {
  for (double** p : {&ws->w, &ws->z, &ws->V, &ws->Z, &ws->d_h, &ws->d_y, &ws->d_scratch}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  if (ws->h_pin) (void)hipHostFree(ws->h_pin);
  ws->h_pin = nullptr;
  ws->n = ws->ld = 0;
  ws->cap = ws->vcols = ws->zcols = ws->hcap = 0;
}

int grow_ws(SolverWs* ws, int64_t n, int k, int vcols, int zcols) {
  const int64_t ld = (n + 1) & ~int64_t(1);                      // even stride: every vector of every system on a 16-byte boundary
  if (ws->n != n || ws->cap < k) {
    reset_ws(ws);
    TRY(grow(&ws->w, (size_t)ld * k));
    TRY(grow(&ws->z, (size_t)ld * k));
    ws->n = n; ws->ld = ld; ws->cap = k;
  }
  const size_t col = (size_t)ld * ws->cap;
  if (ws->vcols < vcols) { ws->vcols = 0; TRY(grow(&ws->V, col * vcols)); ws->vcols = vcols; }
  if (ws->zcols < zcols) { ws->zcols = 0; TRY(grow(&ws->Z, col * zcols)); ws->zcols = zcols; }
  if (ws->hcap < vcols + 1) {
    const int hcap = vcols + 1;
    ws->hcap = 0;
    TRY(grow(&ws->d_h, (size_t)hcap * ws->cap));
    TRY(grow(&ws->d_y, (size_t)hcap * ws->cap));
    TRY(grow(&ws->d_scratch, (size_t)fmmbem_mgs_scratch_doubles(hcap) * ws->cap));
    if (ws->h_pin) (void)hipHostFree(ws->h_pin);
    ws->h_pin = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ws->h_pin), sizeof(double) * 2 * (size_t)hcap * ws->cap, hipHostMallocDefault));
    ws->hcap = hcap;                                             // sizes are committed only once every buffer of the group exists
  }
  return FMMBEM_OK;
}

SolverWs* plan_ws(SolverWs** slot, int device) {
  if (!*slot) { *slot = new SolverWs; (*slot)->device = device; }
  return *slot;
}

// the workspace a plan keeps between solves (an inner-plan preconditioner solves once per outer iteration: no allocation
// there), wide enough for k systems; a failed allocation leaves it empty
int ensure_ws(SolverWs** slot, int device, int64_t n, int k, int vcols, int zcols, SolverWs** out) {
  SolverWs* ws = plan_ws(slot, device);
  const int rc = grow_ws(ws, n, k, vcols, zcols);
  if (rc != FMMBEM_OK) { reset_ws(ws); return rc; }
  *out = ws;
  return FMMBEM_OK;
}

int sweep_grid(int64_t n) {
  const int64_t want = (n + kThreads - 1) / kThreads;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, kBlocks));
}

// SolverOptions::predict_p (SolverOptions.hpp:25-38), the (unsigned) cast of the reference kept as far as it matters: a
// non-positive residual estimate saturates nu at 1 and asks for order 0, which every call site then raises to its floor
int predict_p(const fmmbem_solver_options& o, double eps) {
  if (!o.variable_p) return o.max_p;
  if (!(eps > 0.0)) return o.relax_type == FMMBEM_RELAX_BOURAS ? 0 : o.max_p;
  double v;
  if (o.relax_type == FMMBEM_RELAX_BOURAS) {
    const double alpha = 1.0 / std::min(eps, 1.0);
    const double nu = std::min(alpha * o.residual, 1.0);
    v = std::ceil(-std::log2(nu));
  } else {
    v = std::ceil(-std::log2(eps));
  }
  if (v < 0) return o.max_p;                                     // (unsigned)negative is huge: min(., max_p)
  return v > (double)o.max_p ? o.max_p : (int)v;
}

int order_for(const fmmbem_solver_options& o, double resid, int plan_pmax) {
  const int pp = predict_p(o, std::fabs(resid));
  int p;
  switch (o.order_rule) {
    case FMMBEM_ORDER_GMRES_STOKES: p = std::max(o.p_min, pp - 1); break;      // GMRES_Stokes.hpp:229
    case FMMBEM_ORDER_FGMRES_STOKES: p = std::max(5, pp); break;                // GMRES_Stokes.hpp:373
    default: p = std::max(1, pp); break;                                        // GMRES.hpp:195 (and :324: no order 0 here)
  }
  return std::min(p, plan_pmax);
}

void plane_rotation(double dx, double dy, double* cs, double* sn) {             // GMRES.hpp:88-105 GeneratePlaneRotation
  if (dy == 0.0) { *cs = 1.0; *sn = 0.0; }
  else if (std::fabs(dy) > std::fabs(dx)) { const double t = dx / dy; *sn = 1.0 / std::sqrt(1.0 + t * t); *cs = t * *sn; }
  else { const double t = dy / dx; *cs = 1.0 / std::sqrt(1.0 + t * t); *sn = t * *cs; }
}

// a block-inverse preconditioner (kind 3) without a plan of its own: refused with the null arguments, before the operator
// plan's own refusals (kinds 0-2 keep their order: the plan first)
int check_block_inverse_args(const fmmbem_plan* plan, const fmmbem_preconditioner* M) {
  if (M && M->kind == FMMBEM_PC_BLOCK_INVERSE && (!M->inner_plan || M->inner_plan == plan))
    return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: the preconditioner needs a plan of its own");
  return FMMBEM_OK;
}

// what a solve refuses before it touches anything
int check_solve(fmmbem_plan* plan, const fmmbem_solver_options& so, const fmmbem_preconditioner* M, int depth, int* device, int64_t* n,
                int* plan_pmax, SolverWs*** slot) {
  TRY(fmmbem::plan_solver_info(plan, device, n, plan_pmax, slot));
  if (depth > 1) return fail(FMMBEM_ERR_UNSUPPORTED, "fmmbem_gmres: a preconditioner's inner solve cannot itself be preconditioned by a plan");
  if (so.restart < 1 || so.max_iters < 0 || so.max_p < 1 || !(so.residual > 0.0))
    return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: restart >= 1, max_iters >= 0, max_p >= 1, residual > 0 required");
  const int kind = M ? M->kind : FMMBEM_PC_IDENTITY;
  if (kind == FMMBEM_PC_DIAGONAL && !M->reciprocals) return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: diagonal preconditioner without reciprocals");
  if (kind == FMMBEM_PC_INNER_PLAN) {
    if (!M->inner_plan || M->inner_plan == plan) return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: the preconditioner needs a plan of its own");
    int dv = 0, pm = 0; int64_t nn = 0; SolverWs** sl = nullptr;
    TRY(fmmbem::plan_solver_info(M->inner_plan, &dv, &nn, &pm, &sl));
    if (dv != *device || nn != *n) return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: the preconditioner's plan must hold the same panels on the same device");
  }
  if (kind == FMMBEM_PC_BLOCK_INVERSE) {
    TRY(check_block_inverse_args(plan, M));
    int dv = 0, pm = 0; int64_t nn = 0; SolverWs** sl = nullptr;
    TRY(fmmbem::plan_solver_info(M->inner_plan, &dv, &nn, &pm, &sl));
    if (dv != *device || nn != *n) return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: the preconditioner's plan must hold the same panels on the same device");
    if (!fmmbem::plan_block_inverse_built(M->inner_plan))
      return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: the block-inverse preconditioner's plan has no inverse built (fmmbem_plan_block_inverse_build)");
  }
  if (kind < 0 || kind > FMMBEM_PC_BLOCK_INVERSE) return fail(FMMBEM_ERR_INVALID, "fmmbem_gmres: unknown preconditioner kind");
  return FMMBEM_OK;
}

// The host side of one system: the (R+1) x R Hessenberg matrix, the Givens rotations and the rotated right-hand side
struct Arnoldi {
  int R = 0;
  std::vector<double> H, cs, sn, sv;
  explicit Arnoldi(int restart) : R(restart), H((size_t)(restart + 1) * restart, 0.0), cs(restart, 0.0), sn(restart, 0.0), sv(restart + 1, 0.0) {}
  double& Hm(int r, int c) { return H[(size_t)r * R + c]; }
  // column i arrives (h: i + 2 numbers): the earlier rotations, the new one, the right-hand side (GMRES.hpp:108-117, :214-218)
  void column(int i, const double* h) {
    for (int k = 0; k <= i + 1; ++k) Hm(k, i) = h[k];
    for (int k = 0; k < i; ++k) {          // PlaneRotation, :108-117
      const double t = cs[k] * Hm(k, i) + sn[k] * Hm(k + 1, i);
      Hm(k + 1, i) = -sn[k] * Hm(k, i) + cs[k] * Hm(k + 1, i);
      Hm(k, i) = t;
    }
    plane_rotation(Hm(i, i), Hm(i + 1, i), &cs[i], &sn[i]);
    {
      const double t = cs[i] * Hm(i, i) + sn[i] * Hm(i + 1, i);
      Hm(i + 1, i) = -sn[i] * Hm(i, i) + cs[i] * Hm(i + 1, i);
      Hm(i, i) = t;
    }
    sv[i + 1] = -sn[i] * sv[i];
    sv[i] = cs[i] * sv[i];
  }
  // solve the upper triangular system in place (:228-234): sv[0..i] become the coefficients y
  void back_substitute(int i) {
    for (int j = i; j >= 0; --j) {
      sv[j] /= Hm(j, j);
      for (int k = j - 1; k >= 0; --k) sv[k] -= Hm(k, j) * sv[j];
    }
  }
};

// ================================================================================================================
// The solver: k independent solves of the reference's loop on one plan, advanced in lockstep.  Every system keeps its own
// Krylov space, Hessenberg matrix, rotations, residual estimate and order; restart length and max_iters are common, so the
// systems still running share the column index i and the iteration count.  Per iteration: the matvecs of the systems that ask
// for the same order are one fmmbem_plan_execute_batch_device (the matvec of a one-system solve is fmmbem_plan_execute_device),
// the Arnoldi columns of all of them one chain of i + 3 launches with the system as the grid's second dimension, and their
// Hessenberg columns cross to the host in one copy behind one synchronisation.  No operation on a system's data depends on k or
// on the other systems: a system of a k-system solve gets the bits of its own one-system solve.
// ================================================================================================================
struct System {
  double* x;
  const double* b;
  fmmbem_solver_log* log;
  Arnoldi ar;
  double normb = 0, resid = 0;
  int cur_p = 0;
  System(double* x_, const double* b_, fmmbem_solver_log* log_, int R) : x(x_), b(b_), log(log_), ar(R) {}
};

struct MatvecJob { int p; const double* x; double* y; };

// y = A x for every job of a k-system solve.  k = 1: the single entry point, which replays the plan's graphs when they are on
// (fmmbem_plan_set_graphs); the batch entry point never does.  Otherwise the jobs of one order go through
// fmmbem_plan_execute_batch_device, a lone one included: as many vectors per call as lie equally spaced in x and in y (all of
// a group when it is one column of the workspace and no system between them has left)
int batch_matvecs(fmmbem_plan* plan, int64_t n, int k, const std::vector<MatvecJob>& jobs, hipStream_t s) {
  if (k == 1) return fmmbem_plan_execute_device(plan, jobs[0].p, jobs[0].x, jobs[0].y, s);
  std::vector<char> done(jobs.size(), 0);
  for (size_t a = 0; a < jobs.size(); ++a) {
    if (done[a]) continue;
    std::vector<size_t> g;                                         // the jobs at this order, in system order
    for (size_t c = a; c < jobs.size(); ++c)
      if (!done[c] && jobs[c].p == jobs[a].p) { g.push_back(c); done[c] = 1; }
    for (size_t f = 0; f < g.size();) {
      size_t cnt = 1;
      ptrdiff_t dx = n, dy = n;
      if (f + 1 < g.size()) {
        dx = jobs[g[f + 1]].x - jobs[g[f]].x;
        dy = jobs[g[f + 1]].y - jobs[g[f]].y;
        if (dx >= n && dy >= n) {
          cnt = 2;
          while (f + cnt < g.size() && jobs[g[f + cnt]].x - jobs[g[f + cnt - 1]].x == dx && jobs[g[f + cnt]].y - jobs[g[f + cnt - 1]].y == dy) ++cnt;
        } else {
          dx = dy = n;
        }
      }
      TRY(fmmbem_plan_execute_batch_device(plan, jobs[a].p, (int)cnt, jobs[g[f]].x, (size_t)dx, jobs[g[f]].y, (size_t)dy, s));
      f += cnt;
    }
  }
  return FMMBEM_OK;
}

int solve(fmmbem_plan* plan, const fmmbem_solver_options& so, int k, double* const* xs, const double* const* bs,
          const fmmbem_preconditioner* M, fmmbem_solver_log* const* logs, hipStream_t s, int depth);

struct Solver {
  fmmbem_plan* plan;
  const fmmbem_solver_options& so;
  const fmmbem_preconditioner* M;
  hipStream_t s;
  int depth, kind, plan_pmax;
  int64_t n, ld;
  SolverWs* ws;
  std::vector<System> sys;

  double* wv(int j) const { return ws->w + (int64_t)j * ld; }
  double* Vc(int c, int j) const { return ws->V + ((int64_t)c * ws->cap + j) * ld; }
  double* Zc(int c, int j) const { return ws->Z + ((int64_t)c * ws->cap + j) * ld; }
  double* scratch(int j) const { return ws->d_scratch + (size_t)j * fmmbem_mgs_scratch_doubles(ws->hcap); }

  // a launch per kSysPerLaunch systems: f(table, first position of the table in `act`)
  template <class F> void for_tables(const std::vector<int>& act, F f) const {
    for (size_t a = 0; a < act.size(); a += kSysPerLaunch) {
      SysTable t;
      t.count = (int)std::min<size_t>(kSysPerLaunch, act.size() - a);
      for (int q = 0; q < kSysPerLaunch; ++q) t.slot[q] = q < t.count ? act[a + q] : 0;
      f(t, a);
    }
  }

  // |w| (after w += a v when v) of system j -> host; one synchronisation
  int norm(int j, double* w, double a, const double* v, double* out) const {
    hipLaunchKernelGGL(axpy_norm_kernel, dim3(sweep_grid(n)), dim3(kThreads), 0, s, n, w, a, v, scratch(j));
    hipLaunchKernelGGL(mgs_finish_kernel, dim3(1), dim3(kThreads), 0, s, scratch(j), 0, ws->d_h);      // ncols = 0: row 0 is a norm
    HIP_TRY(hipMemcpyAsync(ws->h_pin, ws->d_h, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = ws->h_pin[0];
    return FMMBEM_OK;
  }

  // z_j = M(column c of system j) for the systems of act -> zs; one launch (diagonal) or one inner solve of all of them
  int apply_pc(const std::vector<int>& act, int c, bool keep, std::vector<const double*>* zs) const {
    zs->clear();
    if (kind == FMMBEM_PC_IDENTITY) {
      for (int j : act) zs->push_back(Vc(c, j));
      return FMMBEM_OK;
    }
    double* out = keep ? Zc(c, 0) : ws->z;                          // system j: j * ld further on, either way
    for (int j : act) zs->push_back(out + (int64_t)j * ld);
    if (kind == FMMBEM_PC_DIAGONAL) {
      for_tables(act, [&](const SysTable& t, size_t) {
        hipLaunchKernelGGL(scale_multi_kernel, dim3(sweep_grid(n), t.count), dim3(kThreads), 0, s, n, Vc(c, 0), M->reciprocals, out, ld, t);
      });
      return FMMBEM_OK;
    }
    if (kind == FMMBEM_PC_BLOCK_INVERSE) {
      // one pass over the inverses per run of neighbouring systems (all of act until one of them has left)
      for (size_t a = 0; a < act.size();) {
        size_t cnt = 1;
        while (a + cnt < act.size() && act[a + cnt] == act[a] + (int)cnt) ++cnt;
        TRY(fmmbem_plan_block_inverse_apply_device(M->inner_plan, (int)cnt, Vc(c, act[a]), (size_t)ld, out + (int64_t)act[a] * ld, (size_t)ld, s));
        a += cnt;
      }
      return FMMBEM_OK;
    }
    // LocalPC.hpp:35-41: fill(y, 0); GMRES(plan, y, x, options) -- for all systems of act in one solve on the inner plan
    std::vector<double*> y;
    std::vector<const double*> v;
    for (int j : act) {
      y.push_back(out + (int64_t)j * ld);
      v.push_back(Vc(c, j));
    }
    // one memset from the first to the last system of act: a system in between that has left has finished with its z
    HIP_TRY(hipMemsetAsync(y.front(), 0, sizeof(double) * (size_t)((int64_t)(act.back() - act.front()) * ld + n), s));
    return solve(M->inner_plan, M->inner, (int)act.size(), y.data(), v.data(), nullptr, nullptr, s, depth + 1);
  }

  // the Arnoldi column of every system of act: fmmbem_mgs_column_device with the system as the grid's second dimension; the
  // columns land in d_h in the order of act, ncols + 1 doubles each
  void mgs_columns(const std::vector<int>& act, int ncols) const {
    const int64_t want = (n / 4 + kThreads - 1) / kThreads + 1;
    const int grid = (int)(want < kBlocks ? want : kBlocks);        // as fmmbem_mgs_column_device: the partial sums depend on it
    const int64_t ps = fmmbem_mgs_scratch_doubles(ws->hcap);
    double* sc = ws->d_scratch;
    for_tables(act, [&](const SysTable& t, size_t first) {
      for (int c = 0; c <= ncols; ++c)
        hipLaunchKernelGGL(mgs_step_multi_kernel, dim3(grid, t.count), dim3(kThreads), 0, s, n, ws->w, c ? Vc(c - 1, 0) : (const double*)nullptr,
                           c ? sc + (size_t)(c - 1) * kBlocks : (const double*)nullptr, c < ncols ? Vc(c, 0) : (const double*)nullptr,
                           sc + (size_t)c * kBlocks, ld, ps, t);
      hipLaunchKernelGGL(mgs_scale_multi_kernel, dim3(grid, t.count), dim3(kThreads), 0, s, n, ws->w, sc + (size_t)ncols * kBlocks, Vc(ncols, 0), ld, ps, t);
      hipLaunchKernelGGL(mgs_finish_multi_kernel, dim3(ncols + 1, t.count), dim3(kThreads), 0, s, sc, ncols, ws->d_h + first * (size_t)(ncols + 1), ps, t);
    });
  }

  // back substitution and x += ... of system j after column i (GMRES.hpp:228-241; FGMRES :368-371)
  int update(int j, int i) {
    System& S = sys[j];
    S.ar.back_substitute(i);
    const int grid = sweep_grid(n);
    if (kind == FMMBEM_PC_INNER_PLAN && !so.flexible) {
      const std::vector<int> one(1, j);
      std::vector<const double*> z;
      for (int c = 0; c <= i; ++c) {           // x += y_c M(V_c): the inner solve again, column by column, as the reference
        TRY(apply_pc(one, c, false, &z));
        hipLaunchKernelGGL(mgs_axpy_kernel, dim3(grid), dim3(kThreads), 0, s, n, S.x, S.ar.sv[c], z[0]);
      }
      return FMMBEM_OK;
    }
    // this system's slice of the pinned y area: rewritten at the earliest one synchronised iteration later
    double* hy = ws->h_pin + (size_t)ws->hcap * (ws->cap + j);
    double* dy = ws->d_y + (size_t)ws->hcap * j;
    for (int c = 0; c <= i; ++c) hy[c] = S.ar.sv[c];
    HIP_TRY(hipMemcpyAsync(dy, hy, sizeof(double) * (size_t)(i + 1), hipMemcpyHostToDevice, s));
    if (kind == FMMBEM_PC_BLOCK_INVERSE && !so.flexible) {
      // M is linear and constant: x += M (sum_c y_c V_c), one pass over the inverses instead of one per column.  The sum is
      // formed in this system's w, which the Arnoldi column has finished with
      HIP_TRY(hipMemsetAsync(wv(j), 0, sizeof(double) * (size_t)n, s));
      hipLaunchKernelGGL(update_x_kernel, dim3(grid), dim3(kThreads), 0, s, n, wv(j), Vc(0, j), ld * ws->cap, i + 1, dy, (const double*)nullptr);
      double* zj = ws->z + (int64_t)j * ld;
      TRY(fmmbem_plan_block_inverse_apply_device(M->inner_plan, 1, wv(j), (size_t)ld, zj, (size_t)ld, s));
      hipLaunchKernelGGL(mgs_axpy_kernel, dim3(grid), dim3(kThreads), 0, s, n, S.x, 1.0, zj);
      return FMMBEM_OK;
    }
    // FGMRES with the identity: Z_c = V_c was never copied (apply_pc hands V_c back), the update reads V
    hipLaunchKernelGGL(update_x_kernel, dim3(grid), dim3(kThreads), 0, s, n, S.x, (so.flexible && kind != FMMBEM_PC_IDENTITY) ? Zc(0, j) : Vc(0, j), ld * ws->cap, i + 1, dy,
                       (!so.flexible && kind == FMMBEM_PC_DIAGONAL) ? M->reciprocals : (const double*)nullptr);
    return FMMBEM_OK;
  }

  int run() {
    const int R = so.restart;
    const int k = (int)sys.size();
    std::vector<int> live;
    for (int j = 0; j < k; ++j) {
      System& S = sys[j];
      if (S.log) { S.log->iterations = 0; S.log->residual = 0.0; }
      TRY(norm(j, const_cast<double*>(S.b), 0.0, nullptr, &S.normb));      // scale residual by |b| (GMRES.hpp:162)
      if (S.normb == 0.0) continue;            // b = 0: the reference divides by zero and stops on NaN; x = x0 is returned
      S.cur_p = std::min(so.initial_p > 0 ? so.initial_p : so.max_p, plan_pmax);
      live.push_back(j);
    }
    int iter = 0;
    const auto finish = [&](int j) {
      if (sys[j].log) { sys[j].log->iterations = iter; sys[j].log->residual = std::fabs(sys[j].resid); }
    };
    std::vector<MatvecJob> jobs;
    std::vector<const double*> zs;
    while (!live.empty()) {                    // outer (restart) loop, :166 -- the systems still running restart together
      jobs.clear();
      for (int j : live) jobs.push_back({sys[j].cur_p, sys[j].x, wv(j)});      // w = A x at each system's current order
      TRY(batch_matvecs(plan, n, k, jobs, s));
      std::vector<int> act;
      for (int j : live) {
        System& S = sys[j];
        double beta = 0;
        TRY(norm(j, wv(j), -1.0, S.b, &beta));                             // w -= b; beta = |w|
        if (beta == 0.0) { S.resid = 0.0; finish(j); continue; }               // x solves the system exactly
        hipLaunchKernelGGL(scale_kernel, dim3(sweep_grid(n)), dim3(kThreads), 0, s, n, wv(j), -1.0 / beta, Vc(0, j));   // V_0 = -w / beta
        S.ar.sv[0] = beta;
        S.resid = S.ar.sv[0] / S.normb;
        act.push_back(j);
      }
      if (act.empty()) break;
      int i = -1;
      for (;;) {                               // inner loop, :186 -- one column of every system of act
        ++i;
        ++iter;
        for (int j : act) sys[j].cur_p = order_for(so, sys[j].resid, plan_pmax);
        TRY(apply_pc(act, i, so.flexible != 0, &zs));
        jobs.clear();
        for (size_t a = 0; a < act.size(); ++a) jobs.push_back({sys[act[a]].cur_p, zs[a], wv(act[a])});
        TRY(batch_matvecs(plan, n, k, jobs, s));
        // modified Gram-Schmidt against V_0..V_i, |w|, V_{i+1} = w / |w| (:203-212), then the columns to the host
        mgs_columns(act, i + 1);
        HIP_TRY(hipMemcpyAsync(ws->h_pin, ws->d_h, sizeof(double) * (size_t)(i + 2) * act.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int> stay;
        for (size_t a = 0; a < act.size(); ++a) {
          const int j = act[a];
          System& S = sys[j];
          S.ar.column(i, ws->h_pin + a * (size_t)(i + 2));
          S.resid = S.ar.sv[i + 1] / S.normb;
          if (S.log && S.log->p && S.log->resid && iter <= S.log->capacity) { S.log->p[iter - 1] = S.cur_p; S.log->resid[iter - 1] = std::fabs(S.resid); }
          if (std::fabs(S.resid) > so.residual) { stay.push_back(j); continue; }
          TRY(update(j, i));               // converged (or not a number): this system's solve ends here
          finish(j);
        }
        act.swap(stay);
        if (act.empty() || !(i + 1 < R && i + 1 <= so.max_iters)) break;      // :221
      }
      for (int j : act) TRY(update(j, i));
      if (iter < so.max_iters) { live.swap(act); continue; }
      for (int j : act) finish(j);
      break;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return hipGetLastError() == hipSuccess ? FMMBEM_OK : fail(FMMBEM_ERR_HIP, "fmmbem_gmres: a launch failed");
  }
};

int solve(fmmbem_plan* plan, const fmmbem_solver_options& so, int k, double* const* xs, const double* const* bs,
          const fmmbem_preconditioner* M, fmmbem_solver_log* const* logs, hipStream_t s, int depth) {
  int device = 0, plan_pmax = 0;
  int64_t n = 0;
  SolverWs** slot = nullptr;
  TRY(check_solve(plan, so, M, depth, &device, &n, &plan_pmax, &slot));
  // the inner loop runs while i + 1 < R and i + 1 <= max_iters (GMRES.hpp:221): at most min(R, max_iters + 1) columns
  const int most = (int)std::min<int64_t>(so.restart, (int64_t)so.max_iters + 1);
  SolverWs* ws = nullptr;
  TRY(ensure_ws(slot, device, n, k, most + 1, so.flexible ? most : 0, &ws));
  Solver S{plan, so, M, s, depth, M ? M->kind : FMMBEM_PC_IDENTITY, plan_pmax, n, ws->ld, ws, {}};
  S.sys.reserve((size_t)k);
  for (int j = 0; j < k; ++j) S.sys.emplace_back(xs[j], bs[j], logs ? logs[j] : nullptr, so.restart);
  return S.run();
}

// the k systems of an entry point: vectors ldx / ldb apart on the device, logs one after the other
int solve_strided(fmmbem_plan* plan, const fmmbem_solver_options& so, int k, double* d_x, size_t ldx, const double* d_b, size_t ldb,
                  const fmmbem_preconditioner* M, fmmbem_solver_log* logs, hipStream_t s) {
  std::vector<double*> xs((size_t)k);
  std::vector<const double*> bs((size_t)k);
  std::vector<fmmbem_solver_log*> lg((size_t)k, nullptr);
  for (int j = 0; j < k; ++j) { xs[j] = d_x + (size_t)j * ldx; bs[j] = d_b + (size_t)j * ldb; if (logs) lg[j] = logs + j; }
  return solve(plan, so, k, xs.data(), bs.data(), M, lg.data(), s, 0);
}

int entry_args(const fmmbem_plan* plan, const fmmbem_solver_options* opts, int k, const void* x, size_t ldx, const void* b, size_t ldb,
               const char* who) {
  if (!plan || !opts || !x || !b) return fail(FMMBEM_ERR_INVALID, std::string(who) + ": null argument");
  if (k < 1) return fail(FMMBEM_ERR_INVALID, std::string(who) + ": k < 1 systems");
  if (ldx < fmmbem::plan_unknowns(plan) || ldb < fmmbem::plan_unknowns(plan))
    return fail(FMMBEM_ERR_INVALID, std::string(who) + ": leading dimension shorter than a vector");
  return FMMBEM_OK;
}

// the device-pointer entry points; log->seconds is the wall time of the call, set even when the solve fails
int gmres_device(fmmbem_plan* plan, const fmmbem_solver_options* opts, int k, double* d_x, size_t ldx, const double* d_b, size_t ldb,
                 const fmmbem_preconditioner* M, fmmbem_solver_log* logs, void* stream, const char* who) {
  TRY(entry_args(plan, opts, k, d_x, ldx, d_b, ldb, who));
  TRY(check_block_inverse_args(plan, M));
  int device = 0, pm = 0; int64_t n = 0; SolverWs** slot = nullptr;
  TRY(fmmbem::plan_solver_info(plan, &device, &n, &pm, &slot));
  DeviceGuard guard(device);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = solve_strided(plan, *opts, k, d_x, ldx, d_b, ldb, M, logs, static_cast<hipStream_t>(stream));
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (logs) for (int j = 0; j < k; ++j) logs[j].seconds = secs;               // the wall time of the call, for every system
  return rc;
}

// the host-pointer entry points: all x, then all b (and the reciprocals of a diagonal preconditioner) staged on the device once
// per solve -- the only PCIe traffic of length n -- in buffers the workspace's reset / grow never touch
int gmres_host(fmmbem_plan* plan, const fmmbem_solver_options* opts, int k, double* x, size_t ldx, const double* b, size_t ldb,
               const fmmbem_preconditioner* M, fmmbem_solver_log* logs, const char* who) {
  TRY(entry_args(plan, opts, k, x, ldx, b, ldb, who));
  TRY(check_block_inverse_args(plan, M));
  int device = 0, pm = 0; int64_t n = 0; SolverWs** slot = nullptr;
  TRY(check_solve(plan, *opts, M, 0, &device, &n, &pm, &slot));          // bad options or preconditioner: before anything is staged
  DeviceGuard guard(device);
  const auto t0 = std::chrono::steady_clock::now();
  SolverWs* ws = plan_ws(slot, device);
  const int64_t ld = (n + 1) & ~int64_t(1);
  const size_t bytes = sizeof(double) * (size_t)n;
  if (ws->xb_doubles < (size_t)2 * k * ld) {
    ws->xb_doubles = 0;
    TRY(grow(&ws->d_xb, (size_t)2 * k * ld));
    ws->xb_doubles = (size_t)2 * k * ld;
  }
  double* d_x = ws->d_xb;
  double* d_b = ws->d_xb + (size_t)k * ld;
  fmmbem_preconditioner Md;
  const fmmbem_preconditioner* Mp = M;
  if (M && M->kind == FMMBEM_PC_DIAGONAL) {
    if (!ws->d_recip) TRY(grow(&ws->d_recip, (size_t)n));                // n is the plan's: allocated once
    HIP_TRY(hipMemcpy(ws->d_recip, M->reciprocals, bytes, hipMemcpyHostToDevice));
    Md = *M;
    Md.reciprocals = ws->d_recip;
    Mp = &Md;
  }
  HIP_TRY(hipMemcpy2D(d_x, sizeof(double) * (size_t)ld, x, sizeof(double) * ldx, bytes, (size_t)k, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(d_b, sizeof(double) * (size_t)ld, b, sizeof(double) * ldb, bytes, (size_t)k, hipMemcpyHostToDevice));
  TRY(solve_strided(plan, *opts, k, d_x, (size_t)ld, d_b, (size_t)ld, Mp, logs, nullptr));
  HIP_TRY(hipMemcpy2D(x, sizeof(double) * ldx, d_x, sizeof(double) * (size_t)ld, bytes, (size_t)k, hipMemcpyDeviceToHost));
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (logs) for (int j = 0; j < k; ++j) logs[j].seconds = secs;
  return FMMBEM_OK;
}

}  // namespace

extern "C" void fmmbem_solver_options_default(fmmbem_solver_options* o) {     // SolverOptions(), SolverOptions.hpp:23
  if (!o) return;
  o->residual = 1e-5; o->max_iters = 500; o->restart = 500; o->max_p = 16; o->p_min = 5; o->variable_p = 1;
  o->relax_type = FMMBEM_RELAX_BOURAS; o->order_rule = FMMBEM_ORDER_GMRES; o->flexible = 0; o->initial_p = 0;
}

// one system: k = 1, the vector's own length as both leading dimensions
extern "C" int fmmbem_gmres_device(fmmbem_plan* plan, const fmmbem_solver_options* opts, double* d_x, const double* d_b,
                                   const fmmbem_preconditioner* M, fmmbem_solver_log* log, void* stream) {
  const size_t n = plan ? fmmbem::plan_unknowns(plan) : 0;
  return gmres_device(plan, opts, 1, d_x, n, d_b, n, M, log, stream, "fmmbem_gmres_device");
}

extern "C" int fmmbem_gmres(fmmbem_plan* plan, const fmmbem_solver_options* opts, double* x, const double* b,
                            const fmmbem_preconditioner* M, fmmbem_solver_log* log) {
  const size_t n = plan ? fmmbem::plan_unknowns(plan) : 0;
  return gmres_host(plan, opts, 1, x, n, b, n, M, log, "fmmbem_gmres");
}

extern "C" int fmmbem_gmres_batch_device(fmmbem_plan* plan, const fmmbem_solver_options* opts, int k, double* d_x, size_t ldx,
                                         const double* d_b, size_t ldb, const fmmbem_preconditioner* M, fmmbem_solver_log* logs, void* stream) {
  return gmres_device(plan, opts, k, d_x, ldx, d_b, ldb, M, logs, stream, "fmmbem_gmres_batch_device");
}

extern "C" int fmmbem_gmres_batch(fmmbem_plan* plan, const fmmbem_solver_options* opts, int k, double* x, size_t ldx,
                                  const double* b, size_t ldb, const fmmbem_preconditioner* M, fmmbem_solver_log* logs) {
  return gmres_host(plan, opts, k, x, ldx, b, ldb, M, logs, "fmmbem_gmres_batch");
}
