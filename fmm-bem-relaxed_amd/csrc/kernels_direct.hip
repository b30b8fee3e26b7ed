// kernels_direct.hip -- the O(N M) Direct sum  y_i = sum_j K(t_i, s_j) x_j  (the reference's Direct::matvec, include/Direct.hpp:232-302)
// with the entries summed where they are made:
//   direct_partial   one lane per target; blockIdx.y picks a chunk of FMMBEM_DIRECT_CHUNK consecutive sources, which the lane walks in
//                    ascending j:  acc = fma(K_ij, x_j, acc)  (Stokes: three accumulators, the 3x3 block applied to x_j in column
//                    order 0, 1, 2); the partial sum goes to part[chunk][target].  K_ij is laplace_entry / stokes_entry of
//                    near_entry.hpp as it stands -- every regime, the self term, the K_fine rule and 1/(2 mu) live there.
//   direct_reduce    y_i = part[0][i] + part[1][i] + ...  in ascending chunk order, over m * W doubles (W = dof, or a quantity's width).
//   direct_field_partial   the same shape for the field quantities at points (gradient, pressure, velocity gradient), below.
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

// The field quantities at points (include/fmmbem.h, "Direct sum: field quantities"): the shape of direct_partial_kernel over the
// quantity's pair function of near_entry.hpp, W = 3, 1, 9 or 6 sums per lane.
//   Gradient           g = laplace_grad_entry;  acc_c = fma(g_c, x_j, acc_c), c = 0, 1, 2
//   Pressure           pi = stokes_pressure_entry;  acc = fma(pi_x, x_j0, acc), then pi_y x_j1, then pi_z x_j2
//   VelocityGradient   stokes_velgrad_far_from / stokes_velgrad_near add the pair, contracted with f = x_j, straight into the nine
//                      sums (the 27 numbers are never formed); the chunk's partial is stored times 1 / (2 mu) -- with one source and
//                      x = e_e the operations of stokes_velgrad_entry
//   Hessian            laplace_hess_entry: acc_c = fma(eta_c, x_j, acc_c) for the six components of the upper triangle, ascending j from
//                      zero sums; the chunk's partial is stored mirrored, nine doubles, so [a][b] and [b][a] are reduced to the same bits
// The K_fine and 16-point rules run in place under the lane mask: a row's order does not depend on a pair's regime.  Points are
// the caller's (m, 3) array; part is [chunk][target][W].  profiles/r28a_direct_field_resources.md has the compiler's report.
constexpr int field_width(FieldQuantity q) { return q == FieldQuantity::Gradient ? 3 : q == FieldQuantity::Pressure ? 1 : 9; }

template <FieldQuantity Q>
__global__ __launch_bounds__(kDirectBlock) void direct_field_partial_kernel(DevicePlan d, int64_t m, const double* __restrict__ pts,
                                                                            const uint8_t* __restrict__ tbc, const double* __restrict__ x,
                                                                            double* __restrict__ part) {
  constexpr int W = field_width(Q);
  const int64_t i = (int64_t)blockIdx.x * kDirectBlock + threadIdx.x;
  if (i >= m) return;
  const V3 t = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  const int64_t N = d.n;
  const int64_t j0 = (int64_t)blockIdx.y * kDirectChunk;
  const int64_t j1 = j0 + kDirectChunk < N ? j0 + kDirectChunk : N;
  double acc[W];
#pragma unroll
  for (int a = 0; a < W; ++a) acc[a] = 0;
  double* out = part + ((int64_t)blockIdx.y * m + i) * W;
  if constexpr (Q == FieldQuantity::Hessian) {
    const int flag = tbc ? (tbc[i] ? 1 : 0) : 0;
    Sym3 h = {0, 0, 0, 0, 0, 0};
    for (int64_t j = j0; j < j1; ++j) laplace_hess_entry(d, t, flag, j, x[j], h);
    out[0] = h.xx; out[1] = h.xy; out[2] = h.xz; out[3] = h.xy; out[4] = h.yy; out[5] = h.yz; out[6] = h.xz; out[7] = h.yz; out[8] = h.zz;
  } else if constexpr (Q == FieldQuantity::Gradient) {
    const int flag = tbc ? (tbc[i] ? 1 : 0) : 0;
    for (int64_t j = j0; j < j1; ++j) {
      const V3 g = laplace_grad_entry(d, t, flag, j);
      const double xj = x[j];
      acc[0] = __builtin_fma(g.x, xj, acc[0]);
      acc[1] = __builtin_fma(g.y, xj, acc[1]);
      acc[2] = __builtin_fma(g.z, xj, acc[2]);
    }
#pragma unroll
    for (int a = 0; a < W; ++a) out[a] = acc[a];
  } else if constexpr (Q == FieldQuantity::Pressure) {
    for (int64_t j = j0; j < j1; ++j) {
      const V3 pi = stokes_pressure_entry(d, t, j);
      acc[0] = __builtin_fma(pi.x, x[3 * j], acc[0]);
      acc[0] = __builtin_fma(pi.y, x[3 * j + 1], acc[0]);
      acc[0] = __builtin_fma(pi.z, x[3 * j + 2], acc[0]);
    }
    out[0] = acc[0];
  } else {
    for (int64_t j = j0; j < j1; ++j) {
      const double A = d.area[j];
      const V3 f = {x[3 * j], x[3 * j + 1], x[3 * j + 2]};
      if (stokes_velgrad_far_from(d, t, V3{d.cx[j], d.cy[j], d.cz[j]}, A,
                                  [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; }, f, acc))
        stokes_velgrad_near(d, t, j, A, f, acc);
    }
    const double sc = 1. / 2 / d.mu;
#pragma unroll
    for (int a = 0; a < W; ++a) out[a] = acc[a] * sc;
  }
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

int direct_field_width(FieldQuantity q) { return field_width(q); }

namespace {

template <FieldQuantity Q>
hipError_t launch_direct_field_as(const DevicePlan& d, int64_t m, const double* pts, const uint8_t* tbc, const double* x, double* part,
                                  double* out, hipStream_t s) {
  constexpr int W = field_width(Q);
  const int64_t nchunks = direct_chunks(d.n);
  const int64_t gx = (m + kDirectBlock - 1) / kDirectBlock, gr = (m * W + kDirectBlock - 1) / kDirectBlock;
  if (nchunks > 65535 || gx > 0x7fffffff || gr > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(direct_field_partial_kernel<Q>, dim3((unsigned)gx, (unsigned)nchunks), dim3(kDirectBlock), 0, s, d, m, pts, tbc, x, part);
  hipLaunchKernelGGL(direct_reduce_kernel<W>, dim3((unsigned)gr), dim3(kDirectBlock), 0, s, part, (int)nchunks, m, out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_direct_field(FieldQuantity q, const DevicePlan& d, int64_t m, const double* pts, const uint8_t* tbc, const double* x,
                               double* part, double* out, hipStream_t s) {
  if (m <= 0 || d.n <= 0) return hipSuccess;
  if ((q == FieldQuantity::Gradient || q == FieldQuantity::Hessian) != (d.dof == 1)) return hipErrorInvalidValue;    // x holds d.dof values per panel
  switch (q) {
    case FieldQuantity::Gradient: return launch_direct_field_as<FieldQuantity::Gradient>(d, m, pts, tbc, x, part, out, s);
    case FieldQuantity::Pressure: return launch_direct_field_as<FieldQuantity::Pressure>(d, m, pts, tbc, x, part, out, s);
    case FieldQuantity::VelocityGradient: return launch_direct_field_as<FieldQuantity::VelocityGradient>(d, m, pts, tbc, x, part, out, s);
    case FieldQuantity::Hessian: return launch_direct_field_as<FieldQuantity::Hessian>(d, m, pts, tbc, x, part, out, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace fmmbem
