// kernels_direct.hip -- the O(N M) Direct sum  y_i = sum_j K(t_i, s_j) x_j  (the reference's Direct::matvec, include/Direct.hpp:232-302)
// with the entries summed where they are made:
//   direct_partial   one lane per target; blockIdx.y picks a chunk of FMMBEM_DIRECT_CHUNK consecutive sources, which the lane walks in
//                    ascending j:  acc = fma(K_ij, x_j, acc)  (Stokes: three accumulators, the 3x3 block applied to x_j in column
//                    order 0, 1, 2); the partial sum goes to part[chunk][target].  K_ij is laplace_entry / stokes_entry of
//                    near_entry.hpp as it stands -- every regime, the self term, the K_fine rule and 1/(2 mu) live there.
//   direct_reduce    y_i = part[0][i] + part[1][i] + ...  in ascending chunk order.
// No atomics, no cross-lane reduction, and the chunk length is a compile-time constant: a result's bits depend on the inputs only,
// not on the number of targets of the call, the launch shape or the run.  All regimes run in ONE pass (profiles/r11a_direct_resources.md
// has the compiler's resource report: no scratch, and the occupancy it leaves).
// The source index j is the same in every lane of a wavefront, so the panel's data and x_j are wave-uniform: the compiler reads them
// with scalar loads through the constant cache; the only per-lane memory traffic is the target point (once) and the partial sum (once).
#include "device_launch.hpp"
#include "near_entry.hpp"

#ifndef FMMBEM_DIRECT_CHUNK
#define FMMBEM_DIRECT_CHUNK 512
#endif

namespace fmmbem {

namespace {

constexpr int kDirectChunk = FMMBEM_DIRECT_CHUNK;
constexpr int kDirectBlock = 256;

// targets: point i = (tx[i * tstride], ty[i * tstride], tz[i * tstride]) -- tstride 3 for the caller's (m, 3) array, 1 for the
// panels' own centroid arrays (the symmetric form); tbc null: every flag 0
template <int DOF>
__global__ __launch_bounds__(kDirectBlock) void direct_partial_kernel(DevicePlan d, int64_t m, const double* __restrict__ tx,
                                                                      const double* __restrict__ ty, const double* __restrict__ tz,
                                                                      int tstride, const uint8_t* __restrict__ tbc,
                                                                      const double* __restrict__ x, double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * kDirectBlock + threadIdx.x;
  if (i >= m) return;
  const V3 t = {tx[i * tstride], ty[i * tstride], tz[i * tstride]};
  const int flag = tbc ? (tbc[i] ? 1 : 0) : 0;
  const int64_t j0 = (int64_t)blockIdx.y * kDirectChunk;
  const int64_t j1 = j0 + kDirectChunk < d.n ? j0 + kDirectChunk : d.n;
  double acc[DOF];
#pragma unroll
  for (int a = 0; a < DOF; ++a) acc[a] = 0;
  for (int64_t j = j0; j < j1; ++j) {
    if constexpr (DOF == 1) {
      acc[0] = __builtin_fma(laplace_entry(d, t, flag, j), x[j], acc[0]);
    } else {
      double b[9];
      stokes_entry(d, t, flag, j, b);
      const double x0 = x[3 * j], x1 = x[3 * j + 1], x2 = x[3 * j + 2];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        acc[a] = __builtin_fma(b[3 * a], x0, acc[a]);
        acc[a] = __builtin_fma(b[3 * a + 1], x1, acc[a]);
        acc[a] = __builtin_fma(b[3 * a + 2], x2, acc[a]);
      }
    }
  }
  double* out = part + ((int64_t)blockIdx.y * m + i) * DOF;
#pragma unroll
  for (int a = 0; a < DOF; ++a) out[a] = acc[a];
}

template <int DOF>
__global__ __launch_bounds__(kDirectBlock) void direct_reduce_kernel(const double* __restrict__ part, int nchunks, int64_t m,
                                                                     double* __restrict__ y) {
  const int64_t k = (int64_t)blockIdx.x * kDirectBlock + threadIdx.x;       // unknown: target * DOF + component
  const int64_t len = m * DOF;
  if (k >= len) return;
  double s = part[k];
  for (int c = 1; c < nchunks; ++c) s += part[(int64_t)c * len + k];
  y[k] = s;
}

}  // namespace

int direct_chunk() { return kDirectChunk; }

int64_t direct_chunks(int64_t n_sources) { return (n_sources + kDirectChunk - 1) / kDirectChunk; }

hipError_t launch_direct(const DevicePlan& d, int64_t m, const double* tx, const double* ty, const double* tz, int tstride,
                         const uint8_t* tbc, const double* x, double* part, double* y, hipStream_t s) {
  if (m <= 0 || d.n <= 0) return hipSuccess;
  const int64_t nchunks = direct_chunks(d.n);
  const int64_t gx = (m + kDirectBlock - 1) / kDirectBlock, gr = (m * d.dof + kDirectBlock - 1) / kDirectBlock;
  if (nchunks > 65535 || gx > 0x7fffffff || gr > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)nchunks), block(kDirectBlock);
  if (d.dof == 3) {
    hipLaunchKernelGGL(direct_partial_kernel<3>, grid, block, 0, s, d, m, tx, ty, tz, tstride, tbc, x, part);
    hipLaunchKernelGGL(direct_reduce_kernel<3>, dim3((unsigned)gr), block, 0, s, part, (int)nchunks, m, y);
  } else {
    hipLaunchKernelGGL(direct_partial_kernel<1>, grid, block, 0, s, d, m, tx, ty, tz, tstride, tbc, x, part);
    hipLaunchKernelGGL(direct_reduce_kernel<1>, dim3((unsigned)gr), block, 0, s, part, (int)nchunks, m, y);
  }
  return hipGetLastError();
}

}  // namespace fmmbem
