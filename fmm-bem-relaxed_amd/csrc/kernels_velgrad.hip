// kernels_velgrad.hip -- the velocity gradient of the Stokes single layer at the points of a field plan
// (fmmbem_plan_execute_velocity_gradient, include/fmmbem.h "Field velocity gradient"): G_i[k][m] = d u'_k / d t_m, nine doubles per
// target, row-major.
//
//   near_velgrad      the near pairs, matrix-free: stokes_velgrad_far_from / stokes_velgrad_near (near_entry.hpp), contracted with f
//   l2p_velgrad       (1 / 2 mu) [ d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3 ] of the local expansions the velocity
//                     execute evaluates; the second derivatives through the DERIVED coefficients, one spherical chain
//   velgrad_scatter   tree order -> distinct points
//   velgrad_entries   fmmbem_kernel_velocity_gradient_entries: the same entry function for independent pairs
//
// A translation unit of its own, as kernels_grad.hip and kernels_pressure.hip: every other kernel keeps its object code.  What it
// needs of kernels_far.hip -- cart2sph, the step tables, the group staging, wave_lds_sync -- is RESTATED here; the arithmetic of the
// recurrence is l2p_stokes_kernel's.
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
// near_velgrad: near_pressure_kernel's form (kernels_pressure.hip).  Lane = target row.  A wavefront takes one target leaf, 64 rows
// at a time, and walks the leaf's runs of source rows in list order, panels ascending, a panel's quadrature points in order: nine
// sums per row in registers, each point's tensor contracted with the panel's f in place (the 27 numbers are never formed), nine
// stores; no atomics, the same bits every run.  A leaf without a near pair stores zeros.
// The source panels' records (centroid, area, the three charges, the K points: 7 + 3 K doubles) are staged through LDS
// [field][panel], a batch of up to 64 consecutive panels of a run at a time.  The K_fine regime runs IN PLACE under the mask of the
// lanes that take it.  The 1 / (2 mu) multiplies a row's nine sums once.
// ---------------------------------------------------------------------------------------------
constexpr int kVgWaves = 4;
constexpr int kVgRecDoubles = 1100;                      // LDS doubles of a wavefront's slice, as kPresRecDoubles
inline int vg_batch(int nq) { const int pb = kVgRecDoubles / (7 + 3 * nq); return pb < 1 ? 1 : pb > kWave ? kWave : pb; }

__global__ __launch_bounds__(kVgWaves * kWave) void near_velgrad_kernel(DevicePlan d, const int64_t n_src, const int PB, double* __restrict__ gt) {
  extern __shared__ double vg_near_lds[];               // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = 7 + 3 * nq;
  const int64_t N = d.n;
  const double sc = 1. / 2 / d.mu;
  double* rec = vg_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kVgWaves + wave; li < nleaf; li += gridDim.x * kVgWaves) {
    const int leaf = __builtin_amdgcn_readfirstlane(d.leaf_begin + li);
    const int row0 = d.leaf_row0[leaf], nrows = d.leaf_nrows[leaf], ncols = d.near_ncols[leaf];
    const int64_t k0 = d.near_ptr[leaf], k1 = d.near_ptr[leaf + 1];
    for (int chunk = 0; chunk < nrows; chunk += kWave) {
      const bool live = chunk + lane < nrows;
      const int64_t i = row0 + (live ? chunk + lane : 0);   // idle lanes take the leaf's first row and store nothing
      const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
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
            const V3 f = {rec[4 * PB + e], rec[5 * PB + e], rec[6 * PB + e]};
            if (stokes_velgrad_far_from(d, t, V3{rec[0 * PB + e], rec[1 * PB + e], rec[2 * PB + e]}, A,
                                        [&](int q) { return V3{rec[(7 + 3 * q) * PB + e], rec[(8 + 3 * q) * PB + e], rec[(9 + 3 * q) * PB + e]}; }, f, acc))
              stokes_velgrad_near(d, t, (int64_t)jb + e, A, f, acc);
          }
        }
      }
      if (live) {
        double* o = gt + 9 * (size_t)(i - n_src);
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = sc * acc[c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// l2p_velgrad: l2p_pressure_kernel's form.  Lane = target row; a wavefront takes a group of the plan's L2P work, stages slots 0..3
// of the group's L in LDS and every lane runs ONE spherical chain over the expansions of order P - 1 that the first derivatives of
// the four potentials are.  With s(n, m) = sqrt((n - |m|)! (n + |m|)!) the coefficient of R_nm (n < P - 1, 0 <= m <= n) of
//     d_z phi        is  fz L_{n+1,m},                                  fz = sqrt((n + 1 - m)(n + 1 + m))
//     (d_x + i d_y)  is  D+ = fp L_{n+1,m-1},                           fp = sqrt((n - m + 1)(n - m + 2))
//     (d_x - i d_y)  is  D- = -fm L_{n+1,m+1},                          fm = sqrt((n + m + 1)(n + m + 2))
// (L_{n,-1} = -conj L_{n,1}), d_x = (D+ + D-) / 2, d_y = (D+ - D-) / (2 i): the tables hold fz, fp / 2, fm / 2.  Per term twelve LDS
// reads (eight at m = 0), then in registers the lane's own combined coefficients
//     W_k = c_k(phi_3) - x_e c_k(phi_e)            k = x, y, z: d_m of the expansion W_k is d_k d_m phi_3 - x_e d_k d_m phi_e
//     A_01 = c_y(phi_0) - c_x(phi_1),  A_02 = c_z(phi_0) - c_x(phi_2),  A_12 = c_z(phi_1) - c_y(phi_2)
// and twelve sums along the recurrence of Ynm and YnmTheta: the spherical gradients of the three W_k (nine) and the values of the
// three A (the antisymmetric part d_m phi_k - d_k phi_m).  Then sph2cart, once, and g_tree[row] += (1 / 2 mu) (...).
// One division by sin a per row; no second derivative by the chain rule.  Order 1 has no term and is not launched.
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

// the step tables of order P1 = P - 1 in m-major step order (fill_pres_tables of kernels_pressure.hip: the same doubles) and the
// three factors of the derived coefficients
__device__ inline void fill_vg_tables(const DevicePlan& d, int P1, int lane, double* sPref, double* sC1, double* sC2, double* sFz, double* sFp, double* sFm) {
  int t = 0;
  for (int m = 0; m < P1; ++m)
    for (int n = m; n < P1; ++n, ++t)
      if ((t & (kWave - 1)) == lane) {
        const double rk = 1.0 / (double)(n - m + 1);
        sPref[t] = d.tabPref[n * n + n + m];
        sC1[t] = n == m ? (double)(2 * m + 1) : (double)(2 * n + 1) * rk;
        sC2[t] = n == m ? 0.0 : (double)(n + m) * rk;
        sFz[t] = sqrt((double)((n + 1 - m) * (n + 1 + m)));
        sFp[t] = 0.5 * sqrt((double)((n - m + 1) * (n - m + 2)));
        sFm[t] = 0.5 * sqrt((double)((n + m + 1) * (n + m + 2)));
      }
}

constexpr int kVgLeaves = 4, kVgL2PWaves = 4, kVgUnrollMax = 12, kVgSlots = 4;   // the groups are cut for l2p_stokes_kernel's 4 leaves

// pres_stage_group of kernels_pressure.hip for slots 0..3: the L of a group's leaves into this wavefront's LDS slice
// [leaf][slot][S]; through the references this lane's leaf within the group, its first lane, the group's rows
__device__ __forceinline__ void vg_stage_group(const DevicePlan& d, int l0, int nl, int S, int lane, double2* Lw,
                                               int& my_leaf, int& my_box, int& my_nr, int& g, int& first, int& total) {
  my_leaf = 0; my_box = 0; my_nr = 0;
  if (lane < nl) { my_leaf = d.l2p_leaf[l0 + lane]; my_box = d.leaf_box[my_leaf]; my_nr = d.leaf_nrows[my_leaf]; }
  const int per = kVgSlots * S, T = nl * per;
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
__global__ __launch_bounds__(kVgL2PWaves * kWave) void l2p_velgrad_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ gt) {
  extern __shared__ double2 vg_lds[];                   // six tables (6 S doubles), then [wave][leaf][slot 0..3][S]
  const int P = PT > 0 ? PT : Prt;
  const int P1 = P - 1;                                 // the order of the derived expansions
  const int S = P * (P + 1) / 2;
  double* sPref = reinterpret_cast<double*>(vg_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  double* sFz = sC2 + S;
  double* sFp = sFz + S;
  double* sFm = sFp + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = vg_lds + 3 * S + (size_t)wave * kVgLeaves * kVgSlots * S;
  if (wave == 0) fill_vg_tables(d, P1, lane, sPref, sC1, sC2, sFz, sFp, sFm);
  __syncthreads();
  const double sc = 1. / 2 / d.mu;
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    vg_stage_group(d, l0, nl, S, lane, Lw, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double2* Ls = Lw + (size_t)(g < 0 ? 0 : g) * kVgSlots * S;
    const double c0 = d.box_center[3 * box], c1 = d.box_center[3 * box + 1], c2 = d.box_center[3 * box + 2];
    for (int chunk = 0; chunk < total; chunk += kWave) {
      const int r_in_leaf = chunk + lane - first;
      if (g < 0 || r_in_leaf >= nrows) continue;
      const int64_t i = row0 + r_in_leaf;
      const double tx = d.cx[i], ty = d.cy[i], tz = d.cz[i];
      const Sph s = cart2sph(tx - c0, ty - c1, tz - c2);
      double gs[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // (d/dr, d/dtheta, d/dphi) of W_x, W_y, W_z
      double av[3] = {0, 0, 0};                              // the values of A_01, A_02, A_12
      double pn = 1, rhom = 1, er = 1, ei = 0, fact = 1;
      const double inv_sa = 1.0 / s.sa, inv_rho = 1.0 / s.rho;
      auto order = [&](int m, int& step, auto unrolled) FMMBEM_INLINE {
        double p = pn, p1 = p, rhon = rhom;
        const double w = m == 0 ? 1.0 : 2.0;
        auto degree = [&](int n) FMMBEM_INLINE {
          int tz_ = 0;                                  // unrolled: a coefficient's LDS reads stay with its term (see l2p_kernel)
          if constexpr (decltype(unrolled)::value)
            asm volatile("" : "+v"(tz_), "+v"(gs[0][0]), "+v"(gs[0][1]), "+v"(gs[0][2]), "+v"(gs[1][0]), "+v"(gs[1][1]), "+v"(gs[1][2]),
                         "+v"(gs[2][0]), "+v"(gs[2][1]), "+v"(gs[2][2]), "+v"(av[0]), "+v"(av[1]), "+v"(av[2]));
          const double *tPref = sPref + tz_, *tC1 = sC1 + tz_, *tC2 = sC2 + tz_, *tFz = sFz + tz_, *tFp = sFp + tz_, *tFm = sFm + tz_;
          const double2* Lm = Ls + tz_;
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
          const double fz = tFz[step], hp = tFp[step], hm = tFm[step];
          const int up = (n + 1) * (n + 2) / 2 + m;                  // (n + 1, m) of the order-P expansions
          double2 cx[kVgSlots], cy[kVgSlots], cz[kVgSlots];          // the derived coefficients of slot e
#pragma unroll
          for (int e = 0; e < kVgSlots; ++e) {
            const double2 Lz = Lm[e * S + up], Lp = Lm[e * S + up + 1];
            double2 Ll;                                              // L_{n+1,m-1}; at m = 0, -conj L_{n+1,1}
            if (m) Ll = Lm[e * S + up - 1];
            else { Ll.x = -Lp.x; Ll.y = Lp.y; }
            const double px = hp * Ll.x, py = hp * Ll.y, mx = hm * Lp.x, my = hm * Lp.y;     // D+ / 2 and -D- / 2
            cx[e].x = px - mx; cx[e].y = py - my;                    // (D+ + D-) / 2
            cy[e].x = py + my; cy[e].y = -(px + mx);                 // (D+ - D-) / (2 i)
            cz[e].x = fz * Lz.x; cz[e].y = fz * Lz.y;
          }
          const double2 W[3] = {{cx[3].x - (tx * cx[0].x + ty * cx[1].x + tz * cx[2].x), cx[3].y - (tx * cx[0].y + ty * cx[1].y + tz * cx[2].y)},
                                {cy[3].x - (tx * cy[0].x + ty * cy[1].x + tz * cy[2].x), cy[3].y - (tx * cy[0].y + ty * cy[1].y + tz * cy[2].y)},
                                {cz[3].x - (tx * cz[0].x + ty * cz[1].x + tz * cz[2].x), cz[3].y - (tx * cz[0].y + ty * cz[1].y + tz * cz[2].y)}};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double re = W[k].x * yr - W[k].y * yi;             // Re(W Ynm)
            gs[k][0] += w * re * factor;
            gs[k][1] += w * (W[k].x * tr - W[k].y * ti);             // Re(W YnmTheta)
            if (m) gs[k][2] += 2 * (-(W[k].x * yi + W[k].y * yr)) * m;   // Re(W Ynm i) m
          }
          const double2 A[3] = {{cy[0].x - cx[1].x, cy[0].y - cx[1].y}, {cz[0].x - cx[2].x, cz[0].y - cx[2].y}, {cz[1].x - cy[2].x, cz[1].y - cy[2].y}};
#pragma unroll
          for (int k = 0; k < 3; ++k) av[k] += w * (A[k].x * yr - A[k].y * yi);
          p1 = pcur; p = pnext;
          rhon *= s.rho;
          ++step;
        };
        if constexpr (decltype(unrolled)::value) {
#pragma unroll
          for (int n = m; n < PT - 1; ++n) degree(n);
        } else {
#pragma nounroll
          for (int n = m; n < P1; ++n) degree(n);
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
        for (int m = 0; m < PT - 1; ++m) order(m, step, std::true_type{});
      } else {
#pragma nounroll
        for (int m = 0; m < P1; ++m) order(m, step, std::false_type{});
      }
      // sph2cart (kernel/LaplaceSpherical.hpp:546-561) of the three gradients: row k of the symmetric part
      const double r = s.rho, st = s.sa, ct = s.ca, cp = s.cb, sp = s.sb;
      double H[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        H[k][0] = st * cp * gs[k][0] + ct * cp / r * gs[k][1] - sp / r / st * gs[k][2];
        H[k][1] = st * sp * gs[k][0] + ct * sp / r * gs[k][1] + cp / r / st * gs[k][2];
        H[k][2] = ct * gs[k][0] - st / r * gs[k][1];
      }
      double* o = gt + 9 * (size_t)(i - n_src);
      o[0] += sc * H[0][0];           o[1] += sc * (H[0][1] + av[0]); o[2] += sc * (H[0][2] + av[1]);
      o[3] += sc * (H[1][0] - av[0]); o[4] += sc * H[1][1];           o[5] += sc * (H[1][2] + av[2]);
      o[6] += sc * (H[2][0] - av[1]); o[7] += sc * (H[2][1] - av[2]); o[8] += sc * H[2][2];
    }
  }
}

// g_points[perm[row]][0..9) = g_tree[row - n_src][0..9): the target rows (tree order) -> the distinct points; one thread per double
__global__ void velgrad_scatter_kernel(const uint32_t* __restrict__ perm, const double* __restrict__ gt, double* __restrict__ out, int64_t n_src, int64_t rows) {
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= 9 * rows) return;
  const int64_t r = u / 9;
  out[(int64_t)perm[n_src + r] * 9 + (u - 9 * r)] = gt[u];
}

// Gamma(target, source) [k][m][e] for m independent pairs: panels [0, m) give the targets (their centroids), [m, 2m) the sources;
// column e is the entry contracted with the unit charge e_e
__global__ void velgrad_entries_kernel(DevicePlan d, int m, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
  const V3 unit[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int e = 0; e < 3; ++e) {
    double G[9];
    stokes_velgrad_entry(d, t, (int64_t)m + i, unit[e], G);
    for (int c = 0; c < 9; ++c) out[27 * (size_t)i + 3 * c + e] = G[c];
  }
}

}  // namespace

hipError_t launch_near_velgrad(const DevicePlan& d, int64_t n_src, double* g_tree, hipStream_t s) {
  const int nleaf = d.leaf_end - d.leaf_begin;
  if (nleaf <= 0) return hipSuccess;
  const int nblk = (nleaf + kVgWaves - 1) / kVgWaves;
  const int pb = vg_batch(d.nq);
  const size_t lds = sizeof(double) * (size_t)kVgWaves * pb * (7 + 3 * d.nq);
  hipLaunchKernelGGL(near_velgrad_kernel, dim3(nblk < 256 * 16 ? nblk : 256 * 16), dim3(kVgWaves * kWave), lds, s, d, n_src, pb, g_tree);
  return hipGetLastError();
}

hipError_t launch_l2p_velgrad(const DevicePlan& d, int p, int64_t n_src, double* g_tree, hipStream_t s) {
  if (d.n_l2p <= 0) return hipSuccess;
  if (p < 1 || p > kPmaxDev || d.nslots < kVgSlots) return hipErrorInvalidValue;
  if (p == 1) return hipSuccess;                       // a constant per box: no gradient
  const int S = p * (p + 1) / 2;
  const size_t per_wave = sizeof(double2) * (size_t)kVgLeaves * kVgSlots * S;           // 34 KB at p = 16
  int nw = (int)((48 * 1024) / per_wave);
  nw = nw < 1 ? 1 : nw > kVgL2PWaves ? kVgL2PWaves : nw;
  const int nblk = (d.n_l2p_grp + nw - 1) / nw;
  const size_t lds = sizeof(double2) * (size_t)(3 * S) + nw * per_wave;
  const dim3 grid(nblk < 256 * 8 ? nblk : 256 * 8), block(nw * kWave);
#define VG_CASE(PP) case PP: hipLaunchKernelGGL(l2p_velgrad_kernel<PP>, grid, block, lds, s, d, p, n_src, g_tree); break;
  switch (p <= kVgUnrollMax ? p : 0) {
    VG_CASE(2) VG_CASE(3) VG_CASE(4) VG_CASE(5) VG_CASE(6) VG_CASE(7) VG_CASE(8)
    VG_CASE(9) VG_CASE(10) VG_CASE(11) VG_CASE(12)
    default: hipLaunchKernelGGL(l2p_velgrad_kernel<0>, grid, block, lds, s, d, p, n_src, g_tree);
  }
#undef VG_CASE
  return hipGetLastError();
}

hipError_t launch_velgrad_scatter(const DevicePlan& d, int64_t n_src, const double* g_tree, double* out, hipStream_t s) {
  const int64_t rows = d.n - n_src;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(velgrad_scatter_kernel, dim3((unsigned)((9 * rows + 255) / 256)), dim3(256), 0, s, d.perm, g_tree, out, n_src, rows);
  return hipGetLastError();
}

hipError_t launch_velgrad_entries(const DevicePlan& d, int m, double* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(velgrad_entries_kernel, dim3((m + 63) / 64), dim3(64), 0, s, d, m, out);
  return hipGetLastError();
}

}  // namespace fmmbem
