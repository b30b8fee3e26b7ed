// kernels_pressure.hip -- the pressure of the Stokes single layer at the points of a field plan (fmmbem_plan_execute_pressure,
// include/fmmbem.h "Field pressure"): q_i = sum_j pi(t_i, s_j) . x_j, one double per target.
//
//   near_pressure      the near pairs, matrix-free (the stored near matrix holds velocities): stokes_pressure_entry (near_entry.hpp)
//   l2p_pressure       - (d_x phi_0 + d_y phi_1 + d_z phi_2) of the local expansions the velocity execute evaluates
//   pressure_scatter   tree order -> distinct points
//   pressure_entries   fmmbem_kernel_pressure_entries: the same entry function for independent pairs
//
// A translation unit of its own: the kernels of the potential execute and of the Laplace gradient keep their object code.  What they
// need of kernels_far.hip -- cart2sph, the step tables, l2p_stage_group, wave_lds_sync -- is RESTATED here as in kernels_grad.hip;
// the arithmetic of a term is l2p_stokes_kernel's.
#include "device_launch.hpp"
#include "launch_choice.hpp"
#include "near_entry.hpp"
#define FMMBEM_INLINE __attribute__((always_inline))

#include <type_traits>

namespace fmmbem {

namespace {

constexpr double kEps = 1e-12;                         // kernel/LaplaceSpherical.hpp:30

__device__ __forceinline__ void wave_lds_sync() {         // kernels_far.hip, restated
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// near_pressure: near_grad_kernel's form (kernels_grad.hip).  Lane = target row.  A wavefront takes one target leaf, 64 rows at a
// time, and walks the leaf's runs of source rows in list order, panels ascending, a panel's quadrature points in order: one sum per
// row in registers, stored once; no atomics, the same bits every run.  A leaf without a near pair stores 0.
// The source panels' records (centroid, area, the three charges, the K points: 7 + 3 K doubles; no normal) are staged through LDS
// [field][panel], a batch of up to 64 consecutive panels of a run at a time.  The K_fine regime runs IN PLACE under the mask of the
// lanes that take it, its vertices fetched from global memory only there; a wavefront whose rows are all far from a panel skips the
// branch.
// ---------------------------------------------------------------------------------------------
constexpr int kPresWaves = 4;
constexpr int kPresRecDoubles = 1100;                    // LDS doubles of a wavefront's slice, as kGradRecDoubles
inline int pres_batch(int nq) { const int pb = kPresRecDoubles / (7 + 3 * nq); return pb < 1 ? 1 : pb > kWave ? kWave : pb; }

__global__ __launch_bounds__(kPresWaves * kWave) void near_pressure_kernel(DevicePlan d, const int64_t n_src, const int PB, double* __restrict__ qt) {
  extern __shared__ double pres_near_lds[];             // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = 7 + 3 * nq;
  const int64_t N = d.n;
  double* rec = pres_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kPresWaves + wave; li < nleaf; li += gridDim.x * kPresWaves) {
    const int leaf = __builtin_amdgcn_readfirstlane(d.leaf_begin + li);
    const int row0 = d.leaf_row0[leaf], nrows = d.leaf_nrows[leaf], ncols = d.near_ncols[leaf];
    const int64_t k0 = d.near_ptr[leaf], k1 = d.near_ptr[leaf + 1];
    for (int chunk = 0; chunk < nrows; chunk += kWave) {
      const bool live = chunk + lane < nrows;
      const int64_t i = row0 + (live ? chunk + lane : 0);   // idle lanes take the leaf's first row and store nothing
      const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
      double acc = 0;
      for (int64_t k = k0; k < k1; ++k) {
        const int j0 = d.near_run_row0[k], off = d.near_run_off[k];
        const int len = (k + 1 < k1 ? d.near_run_off[k + 1] : ncols) - off;
        for (int jb = j0; jb < j0 + len; jb += PB) {
          const int nb = j0 + len - jb < PB ? j0 + len - jb : PB;
          wave_lds_sync();                                // the previous batch's reads are done
          if (lane < nb) {                                // (PB <= 64: one panel per lane)
            const int64_t j = jb + lane;
            rec[0 * PB + lane] = d.cx[j]; rec[1 * PB + lane] = d.cy[j]; rec[2 * PB + lane] = d.cz[j]; rec[3 * PB + lane] = d.area[j];
            rec[4 * PB + lane] = d.xt[3 * j]; rec[5 * PB + lane] = d.xt[3 * j + 1]; rec[6 * PB + lane] = d.xt[3 * j + 2];
            for (int q = 0; q < 3 * nq; ++q) rec[(7 + q) * PB + lane] = d.quad[q * N + j];
          }
          wave_lds_sync();
          for (int e = 0; e < nb; ++e) {
            const double A = rec[3 * PB + e];
            V3 pi;
            if (stokes_pressure_far_from(d, t, V3{rec[0 * PB + e], rec[1 * PB + e], rec[2 * PB + e]}, A,
                                         [&](int q) { return V3{rec[(7 + 3 * q) * PB + e], rec[(8 + 3 * q) * PB + e], rec[(9 + 3 * q) * PB + e]}; }, pi))
              stokes_pressure_near(d, t, (int64_t)jb + e, A, pi);
            acc += pi.x * rec[4 * PB + e] + pi.y * rec[5 * PB + e] + pi.z * rec[6 * PB + e];
          }
        }
      }
      if (live) qt[i - n_src] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// l2p_pressure: l2p_stokes_kernel<false, PT> of kernels_far.hip reduced to what the pressure reads.  Lane = target row; a wavefront
// takes a group of the plan's L2P work (DevicePlan::l2p_grp: <= 4 leaves on a Stokes plan, <= 64 rows; a larger leaf alone, in
// chunks), stages slots 0..2 of the group's L in LDS -- the potentials phi_k with charges f_k, unscaled; slot 3 is not read -- and
// every lane sums, along the recurrence of Ynm and YnmTheta (kernel/LaplaceSpherical.hpp:455-488), the spherical gradients of the
// three expansions: nine sums, terms m-major.  Then sph2cart (:546-561) and q_tree[row] -= d_x phi_0 + d_y phi_1 + d_z phi_2.
// PT > 0: the order at compile time, both loops unrolled; PT = 0: any order.
// ---------------------------------------------------------------------------------------------
struct Sph { double rho, ca, sa, cb, sb; };
__device__ inline Sph cart2sph(double dx, double dy, double dz) {       // kernels_far.hip, restated
  Sph s;
  s.rho = sqrt(dx * dx + dy * dy + dz * dz) + kEps;
  s.ca = dz / s.rho;
  s.sa = sqrt((1.0 - s.ca) * (1.0 + s.ca));
  if (fabs(dx) + fabs(dy) < kEps) { s.cb = 1; s.sb = 0; }
  else if (fabs(dx) < kEps) { s.cb = 0; s.sb = dy > 0 ? 1.0 : -1.0; }
  else { const double h = 1.0 / sqrt(dx * dx + dy * dy); s.cb = dx * h; s.sb = dy * h; }
  return s;
}

// pref = sqrt((n-m)!/(n+m)!) and the Legendre step P_{n+1}^m = c1 x P_n^m - c2 P_{n-1}^m in m-major step order (fill_grad_tables of
// kernels_grad.hip: the same doubles as fill_step_tables of kernels_far.hip)
__device__ inline void fill_pres_tables(const DevicePlan& d, int P, int lane, double* sPref, double* sC1, double* sC2) {
  int t = 0;
  for (int m = 0; m < P; ++m)
    for (int n = m; n < P; ++n, ++t)
      if ((t & (kWave - 1)) == lane) {
        const double rk = 1.0 / (double)(n - m + 1);
        sPref[t] = d.tabPref[n * n + n + m];
        sC1[t] = n == m ? (double)(2 * m + 1) : (double)(2 * n + 1) * rk;
        sC2[t] = n == m ? 0.0 : (double)(n + m) * rk;
      }
}

constexpr int kPresLeaves = 4, kPresL2PWaves = 4, kPresUnrollMax = 12, kPresSlots = 3;   // the groups are cut for l2p_stokes_kernel's 4 leaves

// grad_stage_group of kernels_grad.hip for slots 0..2: the L of a group's leaves into this wavefront's LDS slice [leaf][slot][S];
// through the references this lane's leaf within the group, its first lane, the group's rows
__device__ __forceinline__ void pres_stage_group(const DevicePlan& d, int l0, int nl, int S, int lane, double2* Lw,
                                                 int& my_leaf, int& my_box, int& my_nr, int& g, int& first, int& total) {
  my_leaf = 0; my_box = 0; my_nr = 0;
  if (lane < nl) { my_leaf = d.l2p_leaf[l0 + lane]; my_box = d.leaf_box[my_leaf]; my_nr = d.leaf_nrows[my_leaf]; }
  const int per = kPresSlots * S, T = nl * per;
  constexpr int U = 8;
  for (int e0 = 0; e0 < T; e0 += U * kWave) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * kWave + lane;
      const int ee = e < T ? e : T - 1;
      const int k = ee / per, rem = ee - k * per, a = rem / S, i = rem - a * S;
      const int box = __shfl(my_box, k, kWave);
      v[u] = d.L[((size_t)box * d.nslots + a) * d.s_max + i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * kWave + lane;
      if (e < T) Lw[e] = v[u];
    }
  }
  g = -1; first = 0; total = 0;
  for (int k = 0; k < nl; ++k) {
    const int nr = __shfl(my_nr, k, kWave);
    if (lane >= total && lane < total + nr) { g = k; first = total; }
    total += nr;
  }
}

template <int PT>
__global__ __launch_bounds__(kPresL2PWaves * kWave) void l2p_pressure_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ qt) {
  extern __shared__ double2 pres_lds[];                 // step tables (3 S doubles), then [wave][leaf][slot 0..2][S]
  const int P = PT > 0 ? PT : Prt;
  const int S = P * (P + 1) / 2;
  double* sPref = reinterpret_cast<double*>(pres_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = pres_lds + (3 * S + 1) / 2 + (size_t)wave * kPresLeaves * kPresSlots * S;
  if (wave == 0) fill_pres_tables(d, P, lane, sPref, sC1, sC2);
  __syncthreads();
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    pres_stage_group(d, l0, nl, S, lane, Lw, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double2* Ls = Lw + (size_t)(g < 0 ? 0 : g) * kPresSlots * S;
    const double c0 = d.box_center[3 * box], c1 = d.box_center[3 * box + 1], c2 = d.box_center[3 * box + 2];
    for (int chunk = 0; chunk < total; chunk += kWave) {
      const int r_in_leaf = chunk + lane - first;
      if (g < 0 || r_in_leaf >= nrows) continue;
      const int64_t i = row0 + r_in_leaf;
      const Sph s = cart2sph(d.cx[i] - c0, d.cy[i] - c1, d.cz[i] - c2);
      double gs[kPresSlots][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // (d/dr, d/dtheta, d/dphi) of phi_0..2
      double pn = 1, rhom = 1, er = 1, ei = 0, fact = 1;
      const double inv_sa = 1.0 / s.sa, inv_rho = 1.0 / s.rho;
      auto order = [&](int m, int& step, auto unrolled) FMMBEM_INLINE {
        double p = pn, p1 = p, rhon = rhom;
        const double w = m == 0 ? 1.0 : 2.0;
        auto degree = [&](int n) FMMBEM_INLINE {
          int tz = 0;                                   // unrolled: a coefficient's LDS reads stay with its term (see l2p_kernel)
          if constexpr (decltype(unrolled)::value)
            asm volatile("" : "+v"(tz), "+v"(gs[0][0]), "+v"(gs[0][1]), "+v"(gs[0][2]), "+v"(gs[1][0]), "+v"(gs[1][1]), "+v"(gs[1][2]),
                         "+v"(gs[2][0]), "+v"(gs[2][1]), "+v"(gs[2][2]));
          const double *tPref = sPref + tz, *tC1 = sC1 + tz, *tC2 = sC2 + tz;
          const double2* Lm = Ls + tz;
          const double pref = tPref[step];
          const double mag = rhon * p * pref;
          const double yr = mag * er, yi = mag * ei;                 // Ynm = mag e^{+i m beta}
          const double pcur = p;
          const double pnext = tC1[step] * s.ca * pcur - tC2[step] * p1;
          double tmag;                                               // YnmTheta (LaplaceSpherical.hpp:471,482)
          if (n == m) tmag = rhon * (pnext - (m + 1) * s.ca * pcur) * inv_sa * pref;
          else tmag = rhon * ((n - m + 1) * pnext - (n + 1) * s.ca * pcur) * inv_sa * pref;
          const double tr = tmag * er, ti = tmag * ei;
          const double factor = inv_rho * n;
          const int idx = n * (n + 1) / 2 + m;
#pragma unroll
          for (int e = 0; e < kPresSlots; ++e) {
            const double2 L = Lm[e * S + idx];
            const double re = L.x * yr - L.y * yi;                   // Re(L Ynm)
            gs[e][0] += w * re * factor;
            gs[e][1] += w * (L.x * tr - L.y * ti);                   // Re(L YnmTheta)
            if (m) gs[e][2] += 2 * (-(L.x * yi + L.y * yr)) * m;     // Re(L Ynm i) m
          }
          p1 = pcur; p = pnext;
          rhon *= s.rho;
          ++step;
        };
        if constexpr (decltype(unrolled)::value) {
#pragma unroll
          for (int n = m; n < PT; ++n) degree(n);
        } else {
#pragma nounroll
          for (int n = m; n < P; ++n) degree(n);
        }
        pn = -pn * fact * s.sa;
        fact += 2;
        rhom *= s.rho;
        const double nr = er * s.cb - ei * s.sb, ni = er * s.sb + ei * s.cb;
        er = nr; ei = ni;
      };
      int step = 0;
      if constexpr (PT > 0) {
#pragma unroll
        for (int m = 0; m < PT; ++m) order(m, step, std::true_type{});
      } else {
#pragma nounroll
        for (int m = 0; m < P; ++m) order(m, step, std::false_type{});
      }
      // sph2cart (kernel/LaplaceSpherical.hpp:546-561): component k of grad phi_k, then the trace
      const double r = s.rho, st = s.sa, ct = s.ca, cp = s.cb, sp = s.sb;
      const double dx0 = st * cp * gs[0][0] + ct * cp / r * gs[0][1] - sp / r / st * gs[0][2];
      const double dy1 = st * sp * gs[1][0] + ct * sp / r * gs[1][1] + cp / r / st * gs[1][2];
      const double dz2 = ct * gs[2][0] - st / r * gs[2][1];
      qt[i - n_src] -= dx0 + dy1 + dz2;
    }
  }
}

// q_points[perm[row]] = q_tree[row - n_src]: the target rows (tree order) -> the distinct points
__global__ void pressure_scatter_kernel(const uint32_t* __restrict__ perm, const double* __restrict__ qt, double* __restrict__ out, int64_t n_src, int64_t rows) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= rows) return;
  out[perm[n_src + r]] = qt[r];
}

// pi(target, source) for m independent pairs: panels [0, m) give the targets (their centroids), [m, 2m) the sources
__global__ void pressure_entries_kernel(DevicePlan d, int m, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const V3 e = stokes_pressure_entry(d, V3{d.cx[i], d.cy[i], d.cz[i]}, (int64_t)m + i);
  out[3 * (size_t)i] = e.x; out[3 * (size_t)i + 1] = e.y; out[3 * (size_t)i + 2] = e.z;
}

}  // namespace

hipError_t launch_near_pressure(const DevicePlan& d, int64_t n_src, double* q_tree, hipStream_t s) {
  const int nleaf = d.leaf_end - d.leaf_begin;
  if (nleaf <= 0) return hipSuccess;
  const int nblk = (nleaf + kPresWaves - 1) / kPresWaves;
  const int pb = pres_batch(d.nq);
  const size_t lds = sizeof(double) * (size_t)kPresWaves * pb * (7 + 3 * d.nq);
  hipLaunchKernelGGL(near_pressure_kernel, dim3(nblk < 256 * 16 ? nblk : 256 * 16), dim3(kPresWaves * kWave), lds, s, d, n_src, pb, q_tree);
  return hipGetLastError();
}

hipError_t launch_l2p_pressure(const DevicePlan& d, int p, int64_t n_src, double* q_tree, hipStream_t s) {
  if (d.n_l2p <= 0) return hipSuccess;
  if (p < 1 || p > kPmaxDev || d.nslots < kPresSlots) return hipErrorInvalidValue;
  const int S = p * (p + 1) / 2;
  const size_t per_wave = sizeof(double2) * (size_t)kPresLeaves * kPresSlots * S;         // 26 KB at p = 16
  int nw = (int)((48 * 1024) / per_wave);
  nw = nw < 1 ? 1 : nw > kPresL2PWaves ? kPresL2PWaves : nw;
  const int nblk = (d.n_l2p_grp + nw - 1) / nw;
  const size_t lds = sizeof(double2) * (size_t)((3 * S + 1) / 2) + nw * per_wave;
  const dim3 grid(nblk < 256 * 8 ? nblk : 256 * 8), block(nw * kWave);
#define PRES_CASE(PP) case PP: hipLaunchKernelGGL(l2p_pressure_kernel<PP>, grid, block, lds, s, d, p, n_src, q_tree); break;
  switch (p <= kPresUnrollMax ? p : 0) {
    PRES_CASE(1) PRES_CASE(2) PRES_CASE(3) PRES_CASE(4) PRES_CASE(5) PRES_CASE(6) PRES_CASE(7) PRES_CASE(8)
    PRES_CASE(9) PRES_CASE(10) PRES_CASE(11) PRES_CASE(12)
    default: hipLaunchKernelGGL(l2p_pressure_kernel<0>, grid, block, lds, s, d, p, n_src, q_tree);
  }
#undef PRES_CASE
  return hipGetLastError();
}

hipError_t launch_pressure_scatter(const DevicePlan& d, int64_t n_src, const double* q_tree, double* out, hipStream_t s) {
  const int64_t rows = d.n - n_src;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(pressure_scatter_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d.perm, q_tree, out, n_src, rows);
  return hipGetLastError();
}

hipError_t launch_pressure_entries(const DevicePlan& d, int m, double* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(pressure_entries_kernel, dim3((m + 63) / 64), dim3(64), 0, s, d, m, out);
  return hipGetLastError();
}

}  // namespace fmmbem
