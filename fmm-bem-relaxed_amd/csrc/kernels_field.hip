// kernels_field.hip -- the field quantities at the points of a target plan (include/fmmbem.h "Field gradient", "Field pressure",
// "Field velocity gradient", "Field Hessian"), each the sum over the source panels of its own pair function:
//
//   Gradient           g_i = sum_j gamma(t_i, s_j) x_j, three doubles per target; Laplace plans
//   Pressure           q_i = sum_j pi(t_i, s_j) . x_j, one double per target; the Stokes single layer
//   VelocityGradient   G_i[k][m] = d u'_k / d t_m, nine doubles per target, row-major; the Stokes single layer
//   Hessian            H_i[a][b] = sum_j eta_ab(t_i, s_j) x_j, nine doubles per target, row-major and symmetric; Laplace plans
//
// Written once for all of them: wave_lds_sync, cart2sph, the step tables (fill_tables), the group staging (stage_group), the near
// loop for the gradient and the pressure, the scatter, and one launcher per role.  A quantity's own: its pair step, its L2P chain
// and -- the velocity gradient's -- its copy of the near loop; "The L2P kernels" and the specialisation below say why.
//
//   near_field_kernel<Q>      the near pairs, matrix-free (the stored near matrix holds potentials or velocities): Q's pair function
//                             of near_entry.hpp; explicitly specialised for the velocity gradient
//   near_flow_kernel          the pressure's and the velocity gradient's near pairs in one walk (fmmbem_plan_execute_flow), with the
//                             bits of the two kernels above
//   near_representation_kernel<VALUE, GRAD>   both Laplace layers' near pairs, value and gradient, in one walk
//                             (fmmbem_plan_execute_representation); fold_slots_kernel adds its two multipole sets at the leaves
//   l2p_*_kernel<PT>          what a quantity reads of the local expansions the potential execute evaluates, along the spherical
//                             chain: one kernel per quantity over the shared tables and staging
//   field_scatter_kernel<W>   tree order -> distinct points, W doubles per row
//   *_entries_kernel          the fmmbem_kernel_*_entries calls: the same pair functions for independent pairs
//
// A quantity Q is a plain struct of constants and static __device__ functions (GradientQ, PressureQ, VelocityGradientQ, HessianQ below): the
// record of a source panel and what a pair adds to a row's sums for the near kernel; the slots of L, the tables, the order of the
// chain and the kernel for L2P.  Everything is inlined: no call, no pointer in a kernel, no run-time choice.
//
// A translation unit of its own: the kernels of the potential execute (kernels_near.hip, kernels_far.hip) keep their object code.
// What this unit needs of kernels_far.hip -- cart2sph, the step tables, l2p_stage_group, wave_lds_sync -- is restated from
// kernels_far.hip here, once, as m2p_kernel restates l2p_kernel's term loop there, for that reason; the arithmetic of the recurrence
// is l2p_stokes_kernel's.
#include "device_launch.hpp"
#include "launch_choice.hpp"
#include "near_entry.hpp"
#define FMMBEM_INLINE __attribute__((always_inline))

#include <type_traits>

namespace fmmbem {

namespace {

constexpr double kEps = 1e-12;                         // kernel/LaplaceSpherical.hpp:30

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Sph { double rho, ca, sa, cb, sb; };
__device__ inline Sph cart2sph(double dx, double dy, double dz) {
  Sph s;
  s.rho = sqrt(dx * dx + dy * dy + dz * dz) + kEps;
  s.ca = dz / s.rho;
  s.sa = sqrt((1.0 - s.ca) * (1.0 + s.ca));
  if (fabs(dx) + fabs(dy) < kEps) { s.cb = 1; s.sb = 0; }
  else if (fabs(dx) < kEps) { s.cb = 0; s.sb = dy > 0 ? 1.0 : -1.0; }
  else { const double h = 1.0 / sqrt(dx * dx + dy * dy); s.cb = dx * h; s.sb = dy * h; }
  return s;
}

// fields k, k + 1, k + 2 of a panel's record as a point
template <class Field>
__device__ __forceinline__ V3 point(Field&& field, int k) { return V3{field(k), field(k + 1), field(k + 2)}; }

// each quantity's L2P kernels ("The L2P kernels" below)
template <int PT> __global__ void l2p_grad_kernel(DevicePlan d, int Prt, int64_t n_src, double* gt);
template <int PT> __global__ void l2p_pressure_kernel(DevicePlan d, int Prt, int64_t n_src, double* qt);
template <int PT> __global__ void l2p_velgrad_kernel(DevicePlan d, int Prt, int64_t n_src, double* gt);
template <int PT> __global__ void l2p_hessian_kernel(DevicePlan d, int Prt, int64_t n_src, double* ht);

// =============================================================================================
// The quantities.  For the near kernel: kRec doubles of a source panel's record come before its K points (centroid and area, then
// what stage() puts at fields 4 .. kRec - 1); Acc is a row's sums; pair() adds one panel; store() writes a row.  For L2P: kLeaves
// leaves per group (the groups are cut for the plan's potential L2P), slots() expansions per leaf, kTables step tables of which
// fill_extra() fills those past the three of the recurrence, a chain of order P - kDrop.
// =============================================================================================
struct GradientQ {
  static constexpr int kWidth = 3;
  // ---- near: normal and one charge; laplace_grad_from ----
  static constexpr int kRec = 8;
  using Acc = V3;
  static __device__ __forceinline__ int flag(const DevicePlan& d, int64_t i) { return d.bc[i] ? 1 : 0; }
  static __device__ __forceinline__ void stage(const DevicePlan& d, int64_t j, double* rec, int PB, int lane) {
    rec[4 * PB + lane] = d.nx[j]; rec[5 * PB + lane] = d.ny[j]; rec[6 * PB + lane] = d.nz[j]; rec[7 * PB + lane] = d.xt[j];
  }
  template <class Field>
  static __device__ __forceinline__ void pair(const DevicePlan& d, V3 t, int tb, Field&& field, int64_t j, Acc& acc) {
    const int64_t N = d.n;
    const V3 g = laplace_grad_from(t, tb, point(field, 0), field(3), point(field, 4), d.nq, d.qw, [&](int q) FMMBEM_INLINE { return point(field, kRec + 3 * q); },
                                   [&](int a) { return V3{d.vert[(3 * a + 0) * N + j], d.vert[(3 * a + 1) * N + j], d.vert[(3 * a + 2) * N + j]}; });
    const double x = field(7);
    acc.x += g.x * x; acc.y += g.y * x; acc.z += g.z * x;
  }
  static __device__ __forceinline__ void store(const DevicePlan& d, double* o, const Acc& acc) { o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; }
  // ---- L2P: +- the Cartesian gradient of the expansion of the row's slot -- the slot its flag picks, as in l2p_kernel ----
  static constexpr int kLeaves = 8, kTables = 3, kDrop = 0;
  template <int PT> static constexpr auto l2p_kernel() { return l2p_grad_kernel<PT>; }
  static __device__ __forceinline__ void fill_extra(double*, int, int, int, int) {}
  static __host__ __device__ bool plan_ok(const DevicePlan& d) { return d.n_act >= 1 && d.n_act <= 2; }
  static __host__ __device__ __forceinline__ int slots(const DevicePlan& d) { return d.n_act; }
};

// What the two quantities of the Stokes single layer share: a record of three charges and no normal, no flag, slots 0 .. kSlots - 1
// of L unscaled (the potentials phi_k with charges f_k; slot 3 with charge x . f), l2p_stokes_kernel's 4 leaves per group.
template <int kSlots_>
struct StokesLayerQ {
  static constexpr int kSlots = kSlots_;
  static constexpr int kRec = 7;
  static __device__ __forceinline__ int flag(const DevicePlan&, int64_t) { return 0; }
  static __device__ __forceinline__ void stage(const DevicePlan& d, int64_t j, double* rec, int PB, int lane) {
    rec[4 * PB + lane] = d.xt[3 * j]; rec[5 * PB + lane] = d.xt[3 * j + 1]; rec[6 * PB + lane] = d.xt[3 * j + 2];
  }
  static constexpr int kLeaves = 4;
  static __host__ __device__ bool plan_ok(const DevicePlan& d) { return d.nslots >= kSlots; }
  static __host__ __device__ __forceinline__ int slots(const DevicePlan&) { return kSlots; }
};

struct PressureQ : StokesLayerQ<3> {
  static constexpr int kWidth = 1;
  // ---- near: stokes_pressure_far_from / stokes_pressure_near, contracted with f ----
  using Acc = double;
  template <class Field>
  static __device__ __forceinline__ void pair(const DevicePlan& d, V3 t, int, Field&& field, int64_t j, Acc& acc) {
    const double A = field(3);
    V3 pi;
    if (stokes_pressure_far_from(d, t, point(field, 0), A, [&](int q) FMMBEM_INLINE { return point(field, kRec + 3 * q); }, pi)) stokes_pressure_near(d, t, j, A, pi);
    acc += pi.x * field(4) + pi.y * field(5) + pi.z * field(6);
  }
  static __device__ __forceinline__ void store(const DevicePlan& d, double* o, const Acc& acc) { o[0] = acc; }
  // ---- L2P: - (d_x phi_0 + d_y phi_1 + d_z phi_2): the spherical gradients of three expansions, nine sums ----
  static constexpr int kTables = 3, kDrop = 0;
  template <int PT> static constexpr auto l2p_kernel() { return l2p_pressure_kernel<PT>; }
  static __device__ __forceinline__ void fill_extra(double*, int, int, int, int) {}
};

struct VelocityGradientQ : StokesLayerQ<4> {
  static constexpr int kWidth = 9;
  // ---- near: the specialisation near_field_kernel<VelocityGradientQ> below ----
  // ---- L2P ----
  static constexpr int kTables = 6, kDrop = 1;
  template <int PT> static constexpr auto l2p_kernel() { return l2p_velgrad_kernel<PT>; }
  static __device__ __forceinline__ void fill_extra(double* ext, int S, int t, int n, int m) {
    ext[t] = sqrt((double)((n + 1 - m) * (n + 1 + m)));
    ext[S + t] = 0.5 * sqrt((double)((n - m + 1) * (n - m + 2)));
    ext[2 * S + t] = 0.5 * sqrt((double)((n + m + 1) * (n + m + 2)));
  }
};

// The Hessian of the Laplace field: the gradient's record, flag, slots and grouping; six sums per row, the upper triangle, mirrored at
// the store; for L2P the velocity gradient's tables and chain of order P - 1 over the derived coefficients.
struct HessianQ : GradientQ {
  static constexpr int kWidth = 9;
  // ---- near: laplace_hess_from ----
  using Acc = Sym3;
  template <class Field>
  static __device__ __forceinline__ void pair(const DevicePlan& d, V3 t, int tb, Field&& field, int64_t j, Acc& acc) {
    const int64_t N = d.n;
    laplace_hess_from(t, tb, point(field, 0), field(3), point(field, 4), d.nq, d.qw, [&](int q) FMMBEM_INLINE { return point(field, kRec + 3 * q); },
                      [&](int a) { return V3{d.vert[(3 * a + 0) * N + j], d.vert[(3 * a + 1) * N + j], d.vert[(3 * a + 2) * N + j]}; }, field(7), acc);
  }
  static __device__ __forceinline__ void store(const DevicePlan& d, double* o, const Acc& acc) {
    o[0] = acc.xx; o[1] = acc.xy; o[2] = acc.xz; o[3] = acc.xy; o[4] = acc.yy; o[5] = acc.yz; o[6] = acc.xz; o[7] = acc.yz; o[8] = acc.zz;
  }
  // ---- L2P: +- the Hessian of the expansion of the row's slot ----
  static constexpr int kTables = 6, kDrop = 1;
  template <int PT> static constexpr auto l2p_kernel() { return l2p_hessian_kernel<PT>; }
  static __device__ __forceinline__ void fill_extra(double* ext, int S, int t, int n, int m) { VelocityGradientQ::fill_extra(ext, S, t, n, m); }
};

// ---------------------------------------------------------------------------------------------
// near_field_kernel: lane = target row.  A wavefront takes one target leaf, 64 rows at a time, and walks the leaf's runs of source rows
// (near_ptr -> near_run_row0 / near_run_off) in list order, panels ascending, a panel's quadrature points in order: a row's sums in
// registers, stored once; no atomics, the same bits every run.  A leaf without a near pair stores zeros.
// The source panels' records (centroid, area, Q's fields, the K points: kRec + 3 K doubles) are staged through LDS, a batch of up
// to 64 consecutive panels of a run at a time: lane e loads panel e's fields (full-width loads, consecutive addresses), the
// fields go to [field][panel] in the wavefront's slice, and the lanes then read one panel after the other at a uniform address.
// The regimes: the self value and the fine rule on the vertices run IN PLACE, under the mask of the lanes that take them (the
// vertices are fetched only then, from global memory): a row's sum keeps the list order whatever regime a pair is in, which a
// deferred second pass over the near-regime pairs would not.  A wavefront whose rows are all far from a panel -- the rule off the
// surface -- skips the branch; targets hugging the surface pay both branches for the few panels beside them.
// ---------------------------------------------------------------------------------------------
constexpr int kNearWaves = 4;
constexpr int kRecDoubles = 1100;                        // LDS doubles of a wavefront's slice: 64 panels at K = 1, 3, 4; fewer at the larger rules
inline int near_batch(int nf) { const int pb = kRecDoubles / nf; return pb < 1 ? 1 : pb > kWave ? kWave : pb; }

template <class Q>
__global__ __launch_bounds__(kNearWaves * kWave) void near_field_kernel(DevicePlan d, const int64_t n_src, const int PB, double* __restrict__ out) {
  extern __shared__ double field_near_lds[];            // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = Q::kRec + 3 * nq;
  const int64_t N = d.n;
  double* rec = field_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kNearWaves + wave; li < nleaf; li += gridDim.x * kNearWaves) {
    const int leaf = __builtin_amdgcn_readfirstlane(d.leaf_begin + li);
    const int row0 = d.leaf_row0[leaf], nrows = d.leaf_nrows[leaf], ncols = d.near_ncols[leaf];
    const int64_t k0 = d.near_ptr[leaf], k1 = d.near_ptr[leaf + 1];
    for (int chunk = 0; chunk < nrows; chunk += kWave) {
      const bool live = chunk + lane < nrows;
      const int64_t i = row0 + (live ? chunk + lane : 0);   // idle lanes take the leaf's first row and store nothing
      const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
      const int tb = Q::flag(d, i);
      typename Q::Acc acc = {};
      for (int64_t k = k0; k < k1; ++k) {
        const int j0 = d.near_run_row0[k], off = d.near_run_off[k];
        const int len = (k + 1 < k1 ? d.near_run_off[k + 1] : ncols) - off;
        for (int jb = j0; jb < j0 + len; jb += PB) {
          const int nb = j0 + len - jb < PB ? j0 + len - jb : PB;
          wave_lds_sync();                                // the previous batch's reads are done
          if (lane < nb) {                                // (PB <= 64: one panel per lane)
            const int64_t j = jb + lane;
            rec[0 * PB + lane] = d.cx[j]; rec[1 * PB + lane] = d.cy[j]; rec[2 * PB + lane] = d.cz[j]; rec[3 * PB + lane] = d.area[j];
            Q::stage(d, j, rec, PB, lane);
            for (int q = 0; q < 3 * nq; ++q) rec[(Q::kRec + q) * PB + lane] = d.quad[q * N + j];
          }
          wave_lds_sync();
          for (int e = 0; e < nb; ++e) Q::pair(d, t, tb, [&](int f) FMMBEM_INLINE { return rec[f * PB + e]; }, (int64_t)jb + e, acc);
        }
      }
      if (live) Q::store(d, out + Q::kWidth * (size_t)(i - n_src), acc);
    }
  }
}

// The velocity gradient's near kernel: the loop above once more, with its pair step IN PLACE -- stokes_velgrad_far_from /
// stokes_velgrad_near, each point's tensor contracted with the panel's f (the 27 numbers are never formed), nine sums, the
// 1 / (2 mu) once per row.  Through any function around that step, Q::pair or a lambda, the compiler allots this kernel 146 or 154
// registers instead of 122 -- three wavefronts per SIMD instead of four (profiles/r27a_field_quantities.txt).
template <>
__global__ __launch_bounds__(kNearWaves * kWave) void near_field_kernel<VelocityGradientQ>(DevicePlan d, const int64_t n_src, const int PB, double* __restrict__ gt) {
  extern __shared__ double field_near_lds[];            // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = 7 + 3 * nq;
  const int64_t N = d.n;
  const double sc = 1. / 2 / d.mu;
  double* rec = field_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kNearWaves + wave; li < nleaf; li += gridDim.x * kNearWaves) {
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

// The flow execute's near kernel (include/fmmbem.h "Flow execute"): the pressure AND the velocity gradient of a row in one walk
// over its near lists -- the loop above a third time, the 7 + 3 K doubles of a panel staged once, one regime test per pair, and
// per quadrature point one t - y_q, r2 and reciprocal square root feeding pressure_point and velgrad_point (stokes_flow_far_from /
// stokes_flow_near of near_entry.hpp).  q += pi . f per pair in PressureQ::pair's expression, the nine sums scaled by 1 / (2 mu) at
// the store, two stores: the bits of near_field_kernel<PressureQ> and near_field_kernel<VelocityGradientQ>.
__global__ __launch_bounds__(kNearWaves * kWave) void near_flow_kernel(DevicePlan d, const int64_t n_src, const int PB, double* __restrict__ qt,
                                                                       double* __restrict__ gt) {
  extern __shared__ double field_near_lds[];            // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = 7 + 3 * nq;
  const int64_t N = d.n;
  const double sc = 1. / 2 / d.mu;
  double* rec = field_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kNearWaves + wave; li < nleaf; li += gridDim.x * kNearWaves) {
    const int leaf = __builtin_amdgcn_readfirstlane(d.leaf_begin + li);
    const int row0 = d.leaf_row0[leaf], nrows = d.leaf_nrows[leaf], ncols = d.near_ncols[leaf];
    const int64_t k0 = d.near_ptr[leaf], k1 = d.near_ptr[leaf + 1];
    for (int chunk = 0; chunk < nrows; chunk += kWave) {
      const bool live = chunk + lane < nrows;
      const int64_t i = row0 + (live ? chunk + lane : 0);   // idle lanes take the leaf's first row and store nothing
      const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      double q = 0;
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
            for (int qq = 0; qq < 3 * nq; ++qq) rec[(7 + qq) * PB + lane] = d.quad[qq * N + j];
          }
          wave_lds_sync();
          for (int e = 0; e < nb; ++e) {
            const double A = rec[3 * PB + e];
            const V3 f = {rec[4 * PB + e], rec[5 * PB + e], rec[6 * PB + e]};
            V3 pi;
            if (stokes_flow_far_from(d, t, V3{rec[0 * PB + e], rec[1 * PB + e], rec[2 * PB + e]}, A,
                                     [&](int p) { return V3{rec[(7 + 3 * p) * PB + e], rec[(8 + 3 * p) * PB + e], rec[(9 + 3 * p) * PB + e]}; }, f, pi, acc))
              stokes_flow_near(d, t, (int64_t)jb + e, A, f, pi, acc);
            // pi . f as near_field_kernel<PressureQ> is compiled: of PressureQ::pair's sum of three products the y product is the
            // plain one and x, then z, are fused onto it.  Written out, because here the compiler starts from the x product.
            q += fma(pi.z, f.z, fma(pi.x, f.x, pi.y * f.y));
          }
        }
      }
      if (live) {
        qt[i - n_src] = q;
        double* o = gt + 9 * (size_t)(i - n_src);
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = sc * acc[c];
      }
    }
  }
}

// The representation execute's near kernel (include/fmmbem.h "Representation execute"): the single layer of sigma minus the double
// layer of mu at a row's point, value and gradient, in one walk over its near lists -- near_field_kernel's loop with a record of
// 9 + 3 K doubles per panel (centroid, area, normal, sigma_j, mu_j, the K points) staged once, and laplace_representation_from
// (near_entry.hpp) per pair: one regime test, one dx, |dx|^2 and reciprocal square root per quadrature point for all four
// integrands.  The row's flag is not read.  A row's four sums in registers, stored once: phi to pt, the gradient to gt (VALUE /
// GRAD: the outputs asked; the other pointer is not touched).  The batch is this kernel's own (kRepRecDoubles: 64 panels at K = 3,
// where near_batch gives 61); four workgroups' slices fit a CU's LDS, as the other near kernels' do.
constexpr int kRepRec = 9;
constexpr int kRepRecDoubles = 64 * (kRepRec + 9);
inline int representation_batch(int nf) { const int pb = kRepRecDoubles / nf; return pb < 1 ? 1 : pb > kWave ? kWave : pb; }

template <bool VALUE, bool GRAD>
__global__ __launch_bounds__(kNearWaves * kWave) __attribute__((amdgpu_waves_per_eu(VALUE ? 2 : 4))) void near_representation_kernel(DevicePlan d, const int64_t n_src, const int PB, const double* __restrict__ mu_tree,
                                                                                 double* __restrict__ pt, double* __restrict__ gt) {
  extern __shared__ double field_near_lds[];            // [wave][field][PB]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int nq = d.nq, nf = kRepRec + 3 * nq;
  const int64_t N = d.n;
  double* rec = field_near_lds + (size_t)wave * PB * nf;
  const int nleaf = d.leaf_end - d.leaf_begin;
  for (int li = blockIdx.x * kNearWaves + wave; li < nleaf; li += gridDim.x * kNearWaves) {
    const int leaf = __builtin_amdgcn_readfirstlane(d.leaf_begin + li);
    const int row0 = d.leaf_row0[leaf], nrows = d.leaf_nrows[leaf], ncols = d.near_ncols[leaf];
    const int64_t k0 = d.near_ptr[leaf], k1 = d.near_ptr[leaf + 1];
    for (int chunk = 0; chunk < nrows; chunk += kWave) {
      const bool live = chunk + lane < nrows;
      const int64_t i = row0 + (live ? chunk + lane : 0);   // idle lanes take the leaf's first row and store nothing
      const V3 t = {d.cx[i], d.cy[i], d.cz[i]};
      double phi = 0;
      V3 g = {0, 0, 0};
      for (int64_t k = k0; k < k1; ++k) {
        const int j0 = d.near_run_row0[k], off = d.near_run_off[k];
        const int len = (k + 1 < k1 ? d.near_run_off[k + 1] : ncols) - off;
        for (int jb = j0; jb < j0 + len; jb += PB) {
          const int nb = j0 + len - jb < PB ? j0 + len - jb : PB;
          wave_lds_sync();                                // the previous batch's reads are done
          if (lane < nb) {                                // (PB <= 64: one panel per lane)
            const int64_t j = jb + lane;
            rec[0 * PB + lane] = d.cx[j]; rec[1 * PB + lane] = d.cy[j]; rec[2 * PB + lane] = d.cz[j]; rec[3 * PB + lane] = d.area[j];
            rec[4 * PB + lane] = d.nx[j]; rec[5 * PB + lane] = d.ny[j]; rec[6 * PB + lane] = d.nz[j];
            rec[7 * PB + lane] = d.xt[j]; rec[8 * PB + lane] = mu_tree[j];
            for (int q = 0; q < 3 * nq; ++q) rec[(kRepRec + q) * PB + lane] = d.quad[q * N + j];
          }
          wave_lds_sync();
          for (int e = 0; e < nb; ++e) {
            const int64_t j = (int64_t)jb + e;
            auto field = [&](int f) FMMBEM_INLINE { return rec[f * PB + e]; };
            laplace_representation_from<VALUE, GRAD>(t, point(field, 0), field(3), point(field, 4), field(7), field(8), nq, d.qw,
                                                     [&](int q) FMMBEM_INLINE { return point(field, kRepRec + 3 * q); },
                                                     [&](int a) { return V3{d.vert[(3 * a + 0) * N + j], d.vert[(3 * a + 1) * N + j], d.vert[(3 * a + 2) * N + j]}; },
                                                     phi, g);
          }
        }
      }
      if (live) {
        if (VALUE) pt[i - n_src] = phi;
        if (GRAD) { double* o = gt + 3 * (size_t)(i - n_src); o[0] = g.x; o[1] = g.y; o[2] = g.z; }
      }
    }
  }
}

// M of slot 0 += (or, `set`, =) M of slot 1 at the P2M leaves, the first S coefficients: the representation execute folds the two
// layers into one multipole set before the tree passes.  One thread per coefficient.
__global__ void fold_slots_kernel(DevicePlan d, const int S, const int set) {
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= (int64_t)d.n_p2m * S) return;
  const int li = (int)(u / S), idx = (int)(u - (int64_t)li * S);
  const int box = d.leaf_box[d.p2m_leaf[li]];
  double2* m0 = d.M + ((size_t)box * d.nslots + 0) * d.s_max + idx;
  const double2 m1 = d.M[((size_t)box * d.nslots + 1) * d.s_max + idx];
  if (set) *m0 = m1;
  else { const double2 a = *m0; *m0 = double2{a.x + m1.x, a.y + m1.y}; }
}

// ---------------------------------------------------------------------------------------------
// The L2P kernels: lane = target row; a wavefront takes a group of the plan's L2P work (DevicePlan::l2p_grp: <= kLeaves leaves,
// <= 64 rows; a larger leaf alone, in chunks), stages the quantity's slots of the group's L in LDS (stage_group), and every lane
// sums along the recurrence of Ynm and YnmTheta (kernel/LaplaceSpherical.hpp:455-488), terms m-major, what its quantity reads of
// the expansions; then sph2cart (:546-561) and the quantity's combination into the row the near kernel has written.
// PT > 0: the order at compile time, both loops unrolled; PT = 0: any order.
// The tables, the staging and the launch are written once.  The chain is each kernel's OWN text: written once over a per-quantity
// term (profiles/r27a_field_quantities.txt) the three kernels keep their operation counts but not their results' last bits -- which
// product of a sum of two goes into the fused multiply-add follows the order of the instructions the compiler sees -- and identical
// bits come before sharing.
// ---------------------------------------------------------------------------------------------
constexpr int kL2PWaves = 4, kUnrollMax = 12;

// pref = sqrt((n-m)!/(n+m)!) and the Legendre step P_{n+1}^m = c1 x P_n^m - c2 P_{n-1}^m of order PC in m-major step order
// (fill_step_tables of kernels_far.hip; 1 / (n - m + 1) is divided here where that one reads the host's table of reciprocals: the
// same doubles), then Q's tables, S doubles apart
template <class Q>
__device__ inline void fill_tables(const DevicePlan& d, int PC, int S, int lane, double* tab) {
  int t = 0;
  for (int m = 0; m < PC; ++m)
    for (int n = m; n < PC; ++n, ++t)
      if ((t & (kWave - 1)) == lane) {
        const double rk = 1.0 / (double)(n - m + 1);
        tab[t] = d.tabPref[n * n + n + m];
        tab[S + t] = n == m ? (double)(2 * m + 1) : (double)(2 * n + 1) * rk;
        tab[2 * S + t] = n == m ? 0.0 : (double)(n + m) * rk;
        Q::fill_extra(tab + 3 * S, S, t, n, m);
      }
}

// l2p_stage_group of kernels_far.hip without the scale: the L of a group's leaves, `slots` expansions per leaf, into this
// wavefront's LDS slice [leaf][slot][S]; through the references this lane's leaf within the group, its first lane, the group's rows
template <class SlotOf>
__device__ __forceinline__ void stage_group(const DevicePlan& d, int l0, int nl, int slots, int S, int lane, double2* Lw, SlotOf slot_of,
                                            int& my_leaf, int& my_box, int& my_nr, int& g, int& first, int& total) {
  my_leaf = 0; my_box = 0; my_nr = 0;
  if (lane < nl) { my_leaf = d.l2p_leaf[l0 + lane]; my_box = d.leaf_box[my_leaf]; my_nr = d.leaf_nrows[my_leaf]; }
  const int per = slots * S, T = nl * per;
  constexpr int U = 8;
  for (int e0 = 0; e0 < T; e0 += U * kWave) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * kWave + lane;
      const int ee = e < T ? e : T - 1;
      const int k = ee / per, rem = ee - k * per, a = rem / S, i = rem - a * S;
      const int box = __shfl(my_box, k, kWave);
      v[u] = d.L[((size_t)box * d.nslots + slot_of(a)) * d.s_max + i];
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

// l2p_grad: the spherical gradient (d/dr, d/dtheta, d/dphi) of the expansion of the row's slot -- the slot its flag picks, as in
// l2p_kernel; g_tree[row] += the Cartesian gradient (flag 0) or -= (flag 1): the sign with which l2p_kernel adds the value.
template <int PT>
__global__ __launch_bounds__(kL2PWaves * kWave) void l2p_grad_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ gt) {
  extern __shared__ double2 field_lds[];                 // step tables (3 S doubles), then [wave][leaf][active slot][S]
  const int P = PT > 0 ? PT : Prt;
  const int S = P * (P + 1) / 2, na = d.n_act;
  double* sPref = reinterpret_cast<double*>(field_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = field_lds + (3 * S + 1) / 2 + (size_t)wave * GradientQ::kLeaves * na * S;
  if (wave == 0) fill_tables<GradientQ>(d, P, S, lane, sPref);
  __syncthreads();
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    const int act0 = d.act[0], act1 = d.act[1];
    stage_group(d, l0, nl, na, S, lane, Lw, [&](int a) { return a == 0 ? act0 : act1; }, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double c0 = d.box_center[3 * box], c1 = d.box_center[3 * box + 1], c2 = d.box_center[3 * box + 2];
    for (int chunk = 0; chunk < total; chunk += kWave) {
      const int r_in_leaf = chunk + lane - first;
      if (g < 0 || r_in_leaf >= nrows) continue;
      const int64_t i = row0 + r_in_leaf;
      const int tb = d.bc[i] ? 1 : 0;
      const double2* Ls = Lw + (size_t)(g * na + (na == 2 ? tb : 0)) * S;
      const Sph s = cart2sph(d.cx[i] - c0, d.cy[i] - c1, d.cz[i] - c2);
      double gr = 0, gth = 0, gph = 0;                  // d/dr, d/dtheta, d/dphi of the expansion
      double pn = 1, rhom = 1, er = 1, ei = 0, fact = 1;
      const double inv_sa = 1.0 / s.sa, inv_rho = 1.0 / s.rho;
      auto order = [&](int m, int& step, auto unrolled) FMMBEM_INLINE {
        double p = pn, p1 = p, rhon = rhom;
        const double w = m == 0 ? 1.0 : 2.0;
        auto degree = [&](int n) FMMBEM_INLINE {
          int tz = 0;                                   // unrolled: a coefficient's LDS reads stay with its term (see l2p_kernel)
          if constexpr (decltype(unrolled)::value) asm volatile("" : "+v"(tz), "+v"(gr), "+v"(gth), "+v"(gph));
          const double *tPref = sPref + tz, *tC1 = sC1 + tz, *tC2 = sC2 + tz;
          const double2 L = (Ls + tz)[n * (n + 1) / 2 + m];
          const double pref = tPref[step];
          const double mag = rhon * p * pref;
          const double yr = mag * er, yi = mag * ei;                 // Ynm = mag e^{+i m beta}
          const double pcur = p;
          const double pnext = tC1[step] * s.ca * pcur - tC2[step] * p1;
          double tmag;                                               // YnmTheta (LaplaceSpherical.hpp:471,482)
          if (n == m) tmag = rhon * (pnext - (m + 1) * s.ca * pcur) * inv_sa * pref;
          else tmag = rhon * ((n - m + 1) * pnext - (n + 1) * s.ca * pcur) * inv_sa * pref;
          const double tr = tmag * er, ti = tmag * ei;
          const double re = L.x * yr - L.y * yi;                     // Re(L Ynm)
          gr += w * re * (inv_rho * n);
          gth += w * (L.x * tr - L.y * ti);                          // Re(L YnmTheta)
          if (m) gph += 2 * (-(L.x * yi + L.y * yr)) * m;            // Re(L Ynm i) m
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
      // sph2cart (kernel/LaplaceSpherical.hpp:546-561)
      const double r = s.rho, st = s.sa, ct = s.ca, cp = s.cb, sp = s.sb;
      const double gx = st * cp * gr + ct * cp / r * gth - sp / r / st * gph;
      const double gy = st * sp * gr + ct * sp / r * gth + cp / r / st * gph;
      const double gz = ct * gr - st / r * gth;
      double* o = gt + 3 * (size_t)(i - n_src);
      o[0] += tb ? -gx : gx; o[1] += tb ? -gy : gy; o[2] += tb ? -gz : gz;
    }
  }
}

// l2p_pressure: l2p_stokes_kernel<false, PT> of kernels_far.hip reduced to what the pressure reads: slots 0..2 of L -- the potentials
// phi_k with charges f_k, unscaled; slot 3 is not read --, the spherical gradients of the three expansions, nine sums; then
// q_tree[row] -= d_x phi_0 + d_y phi_1 + d_z phi_2.
template <int PT>
__global__ __launch_bounds__(kL2PWaves * kWave) void l2p_pressure_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ qt) {
  extern __shared__ double2 field_lds[];                 // step tables (3 S doubles), then [wave][leaf][slot 0..2][S]
  const int P = PT > 0 ? PT : Prt;
  const int S = P * (P + 1) / 2;
  double* sPref = reinterpret_cast<double*>(field_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = field_lds + (3 * S + 1) / 2 + (size_t)wave * PressureQ::kLeaves * PressureQ::kSlots * S;
  if (wave == 0) fill_tables<PressureQ>(d, P, S, lane, sPref);
  __syncthreads();
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    stage_group(d, l0, nl, PressureQ::kSlots, S, lane, Lw, [](int a) { return a; }, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double2* Ls = Lw + (size_t)(g < 0 ? 0 : g) * PressureQ::kSlots * S;
    const double c0 = d.box_center[3 * box], c1 = d.box_center[3 * box + 1], c2 = d.box_center[3 * box + 2];
    for (int chunk = 0; chunk < total; chunk += kWave) {
      const int r_in_leaf = chunk + lane - first;
      if (g < 0 || r_in_leaf >= nrows) continue;
      const int64_t i = row0 + r_in_leaf;
      const Sph s = cart2sph(d.cx[i] - c0, d.cy[i] - c1, d.cz[i] - c2);
      double gs[PressureQ::kSlots][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // (d/dr, d/dtheta, d/dphi) of phi_0..2
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
          for (int e = 0; e < PressureQ::kSlots; ++e) {
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

// l2p_velgrad: slots 0..3 of L; g_tree[row] += (1 / 2 mu) [ d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3 ], the second derivatives
// through the DERIVED coefficients: ONE spherical chain over the expansions of order P - 1 that the first derivatives of the four
// potentials are.  With s(n, m) = sqrt((n - |m|)! (n + |m|)!) the coefficient of R_nm (n < P - 1, 0 <= m <= n) of
//     d_z phi        is  fz L_{n+1,m},                                  fz = sqrt((n + 1 - m)(n + 1 + m))
//     (d_x + i d_y)  is  D+ = fp L_{n+1,m-1},                           fp = sqrt((n - m + 1)(n - m + 2))
//     (d_x - i d_y)  is  D- = -fm L_{n+1,m+1},                          fm = sqrt((n + m + 1)(n + m + 2))
// (L_{n,-1} = -conj L_{n,1}), d_x = (D+ + D-) / 2, d_y = (D+ - D-) / (2 i): the three extra tables hold fz, fp / 2, fm / 2.  Per
// term twelve LDS reads (eight at m = 0), then in registers the lane's own combined coefficients
//     W_k = c_k(phi_3) - x_e c_k(phi_e)            k = x, y, z: d_m of the expansion W_k is d_k d_m phi_3 - x_e d_k d_m phi_e
//     A_01 = c_y(phi_0) - c_x(phi_1),  A_02 = c_z(phi_0) - c_x(phi_2),  A_12 = c_z(phi_1) - c_y(phi_2)
// and twelve sums: the spherical gradients of the three W_k (nine) and the values of the three A (the antisymmetric part
// d_m phi_k - d_k phi_m).  Then sph2cart, once.  One division by sin a per row; no second derivative by the chain rule.  Order 1
// has no term and is not launched.
template <int PT>
__global__ __launch_bounds__(kL2PWaves * kWave) void l2p_velgrad_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ gt) {
  extern __shared__ double2 field_lds[];                   // six tables (6 S doubles), then [wave][leaf][slot 0..3][S]
  const int P = PT > 0 ? PT : Prt;
  const int P1 = P - 1;                                 // the order of the derived expansions
  const int S = P * (P + 1) / 2;
  double* sPref = reinterpret_cast<double*>(field_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  double* sFz = sC2 + S;
  double* sFp = sFz + S;
  double* sFm = sFp + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = field_lds + 3 * S + (size_t)wave * VelocityGradientQ::kLeaves * VelocityGradientQ::kSlots * S;
  if (wave == 0) fill_tables<VelocityGradientQ>(d, P1, S, lane, sPref);
  __syncthreads();
  const double sc = 1. / 2 / d.mu;
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    stage_group(d, l0, nl, VelocityGradientQ::kSlots, S, lane, Lw, [](int a) { return a; }, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double2* Ls = Lw + (size_t)(g < 0 ? 0 : g) * VelocityGradientQ::kSlots * S;
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
          double2 cx[VelocityGradientQ::kSlots], cy[VelocityGradientQ::kSlots], cz[VelocityGradientQ::kSlots];          // the derived coefficients of slot e
#pragma unroll
          for (int e = 0; e < VelocityGradientQ::kSlots; ++e) {
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

// l2p_hessian: the Hessian of the expansion of the row's slot -- the slot its flag picks, as in l2p_grad_kernel, whose grouping and
// staging this is -- along l2p_velgrad_kernel's chain: the derived coefficients c_x, c_y, c_z of d_x phi, d_y phi, d_z phi (order
// P - 1; the tables fz, fp / 2, fm / 2), here W_k = c_k(phi_slot) and no antisymmetric part; nine sums, the spherical gradients of the
// three W_k; one division by sin a per row, then sph2cart.  Of the nine Cartesian numbers the upper triangle is kept, component m of
// grad d_k phi for k <= m, and h_tree[row] += it (flag 0) or -= (flag 1), mirrored: [a][b] and [b][a] get the same bits.  Order 1
// has no term and is not launched.
template <int PT>
__global__ __launch_bounds__(kL2PWaves * kWave) void l2p_hessian_kernel(DevicePlan d, const int Prt, const int64_t n_src, double* __restrict__ ht) {
  extern __shared__ double2 field_lds[];                   // six tables (6 S doubles), then [wave][leaf][active slot][S]
  const int P = PT > 0 ? PT : Prt;
  const int P1 = P - 1;                                 // the order of the derived expansions
  const int S = P * (P + 1) / 2, na = d.n_act;
  double* sPref = reinterpret_cast<double*>(field_lds);
  double* sC1 = sPref + S;
  double* sC2 = sC1 + S;
  double* sFz = sC2 + S;
  double* sFp = sFz + S;
  double* sFm = sFp + S;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  double2* Lw = field_lds + 3 * S + (size_t)wave * HessianQ::kLeaves * na * S;
  if (wave == 0) fill_tables<HessianQ>(d, P1, S, lane, sPref);
  __syncthreads();
  for (int gi = blockIdx.x * nwaves + wave; gi < d.n_l2p_grp; gi += gridDim.x * nwaves) {
    const int l0 = d.l2p_grp[gi], nl = d.l2p_grp[gi + 1] - l0;
    wave_lds_sync();                                    // the previous group's reads are done
    int g, first, total, my_leaf, my_box, my_nr;
    const int act0 = d.act[0], act1 = d.act[1];
    stage_group(d, l0, nl, na, S, lane, Lw, [&](int a) { return a == 0 ? act0 : act1; }, my_leaf, my_box, my_nr, g, first, total);
    wave_lds_sync();
    if (nl == 1) { g = 0; first = 0; }                  // single leaf: every lane, chunk by chunk
    const int leaf = __shfl(my_leaf, g < 0 ? 0 : g, kWave), box = __shfl(my_box, g < 0 ? 0 : g, kWave);
    const int row0 = d.leaf_row0[leaf], nrows = __shfl(my_nr, g < 0 ? 0 : g, kWave);
    const double c0 = d.box_center[3 * box], c1 = d.box_center[3 * box + 1], c2 = d.box_center[3 * box + 2];
    for (int chunk = 0; chunk < total; chunk += kWave) {
      const int r_in_leaf = chunk + lane - first;
      if (g < 0 || r_in_leaf >= nrows) continue;
      const int64_t i = row0 + r_in_leaf;
      const int tb = d.bc[i] ? 1 : 0;
      const double2* Ls = Lw + (size_t)(g * na + (na == 2 ? tb : 0)) * S;
      const Sph s = cart2sph(d.cx[i] - c0, d.cy[i] - c1, d.cz[i] - c2);
      double gs[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // (d/dr, d/dtheta, d/dphi) of d_x phi, d_y phi, d_z phi
      double pn = 1, rhom = 1, er = 1, ei = 0, fact = 1;
      const double inv_sa = 1.0 / s.sa, inv_rho = 1.0 / s.rho;
      auto order = [&](int m, int& step, auto unrolled) FMMBEM_INLINE {
        double p = pn, p1 = p, rhon = rhom;
        const double w = m == 0 ? 1.0 : 2.0;
        auto degree = [&](int n) FMMBEM_INLINE {
          int tz_ = 0;                                  // unrolled: a coefficient's LDS reads stay with its term (see l2p_kernel)
          if constexpr (decltype(unrolled)::value)
            asm volatile("" : "+v"(tz_), "+v"(gs[0][0]), "+v"(gs[0][1]), "+v"(gs[0][2]), "+v"(gs[1][0]), "+v"(gs[1][1]), "+v"(gs[1][2]),
                         "+v"(gs[2][0]), "+v"(gs[2][1]), "+v"(gs[2][2]));
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
          const int up = (n + 1) * (n + 2) / 2 + m;                  // (n + 1, m) of the order-P expansion
          const double2 Lz = Lm[up], Lp = Lm[up + 1];
          double2 Ll;                                                // L_{n+1,m-1}; at m = 0, -conj L_{n+1,1}
          if (m) Ll = Lm[up - 1];
          else { Ll.x = -Lp.x; Ll.y = Lp.y; }
          const double px = hp * Ll.x, py = hp * Ll.y, mx = hm * Lp.x, my = hm * Lp.y;     // D+ / 2 and -D- / 2
          const double2 W[3] = {{px - mx, py - my},                  // (D+ + D-) / 2
                                {py + my, -(px + mx)},               // (D+ - D-) / (2 i)
                                {fz * Lz.x, fz * Lz.y}};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double re = W[k].x * yr - W[k].y * yi;             // Re(W Ynm)
            gs[k][0] += w * re * factor;
            gs[k][1] += w * (W[k].x * tr - W[k].y * ti);             // Re(W YnmTheta)
            if (m) gs[k][2] += 2 * (-(W[k].x * yi + W[k].y * yr)) * m;   // Re(W Ynm i) m
          }
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
      // sph2cart (kernel/LaplaceSpherical.hpp:546-561): component m of grad d_k phi, k <= m
      const double r = s.rho, st = s.sa, ct = s.ca, cp = s.cb, sp = s.sb;
      const double hxx = st * cp * gs[0][0] + ct * cp / r * gs[0][1] - sp / r / st * gs[0][2];
      const double hxy = st * sp * gs[0][0] + ct * sp / r * gs[0][1] + cp / r / st * gs[0][2];
      const double hxz = ct * gs[0][0] - st / r * gs[0][1];
      const double hyy = st * sp * gs[1][0] + ct * sp / r * gs[1][1] + cp / r / st * gs[1][2];
      const double hyz = ct * gs[1][0] - st / r * gs[1][1];
      const double hzz = ct * gs[2][0] - st / r * gs[2][1];
      const double sg = tb ? -1.0 : 1.0;
      double* o = ht + 9 * (size_t)(i - n_src);
      const double oxx = o[0] + sg * hxx, oxy = o[1] + sg * hxy, oxz = o[2] + sg * hxz, oyy = o[4] + sg * hyy, oyz = o[5] + sg * hyz, ozz = o[8] + sg * hzz;
      o[0] = oxx; o[1] = oxy; o[2] = oxz; o[3] = oxy; o[4] = oyy; o[5] = oyz; o[6] = oxz; o[7] = oyz; o[8] = ozz;
    }
  }
}

// out[W perm[row] + a] = tree[W (row - n_src) + a]: the target rows (tree order) -> the distinct points; one thread per double
template <int W>
__global__ void field_scatter_kernel(const uint32_t* __restrict__ perm, const double* __restrict__ tree, double* __restrict__ out, int64_t n_src, int64_t rows) {
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u >= W * rows) return;
  const int64_t r = u / W;
  out[W * (int64_t)perm[n_src + r] + (u - W * r)] = tree[u];
}

// The pair functions for m independent pairs: panels [0, m) give the targets (their centroids and flags), [m, 2m) the sources.
// gamma(target, source)
__global__ void grad_entries_kernel(DevicePlan d, int m, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const V3 e = laplace_grad_entry(d, V3{d.cx[i], d.cy[i], d.cz[i]}, d.bc[i] ? 1 : 0, (int64_t)m + i);
  out[3 * (size_t)i] = e.x; out[3 * (size_t)i + 1] = e.y; out[3 * (size_t)i + 2] = e.z;
}

// pi(target, source)
__global__ void pressure_entries_kernel(DevicePlan d, int m, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const V3 e = stokes_pressure_entry(d, V3{d.cx[i], d.cy[i], d.cz[i]}, (int64_t)m + i);
  out[3 * (size_t)i] = e.x; out[3 * (size_t)i + 1] = e.y; out[3 * (size_t)i + 2] = e.z;
}

// Gamma(target, source) [k][m][e]: column e is the entry contracted with the unit charge e_e
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

// eta(target, source), row-major 3x3: the upper triangle mirrored
__global__ void hess_entries_kernel(DevicePlan d, int m, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Sym3 e = {0, 0, 0, 0, 0, 0};
  laplace_hess_entry(d, V3{d.cx[i], d.cy[i], d.cz[i]}, d.bc[i] ? 1 : 0, (int64_t)m + i, 1.0, e);
  double* o = out + 9 * (size_t)i;
  o[0] = e.xx; o[1] = e.xy; o[2] = e.xz; o[3] = e.xy; o[4] = e.yy; o[5] = e.yz; o[6] = e.xz; o[7] = e.yz; o[8] = e.zz;
}

// f(Q{}) for the quantity q names
template <class F>
hipError_t with_quantity(FieldQuantity q, F&& f) {
  switch (q) {
    case FieldQuantity::Gradient: return f(GradientQ{});
    case FieldQuantity::Pressure: return f(PressureQ{});
    case FieldQuantity::VelocityGradient: return f(VelocityGradientQ{});
    case FieldQuantity::Hessian: return f(HessianQ{});
  }
  return hipErrorInvalidValue;
}

template <class Q>
hipError_t launch_l2p(const DevicePlan& d, int p, int64_t n_src, double* tree, hipStream_t s) {
  if (p < 1 || p > kPmaxDev || !Q::plan_ok(d)) return hipErrorInvalidValue;
  if (p <= Q::kDrop) return hipSuccess;                // the chain has no term
  const int S = p * (p + 1) / 2;
  const size_t per_wave = sizeof(double2) * (size_t)Q::kLeaves * Q::slots(d) * S;       // at p = 16: 35 KB (two slots of 8 leaves), 26 KB, 34 KB
  int nw = (int)((48 * 1024) / per_wave);
  nw = nw < 1 ? 1 : nw > kL2PWaves ? kL2PWaves : nw;
  const int nblk = (d.n_l2p_grp + nw - 1) / nw;
  const size_t lds = sizeof(double2) * (size_t)((Q::kTables * S + 1) / 2) + nw * per_wave;
  const dim3 grid(nblk < 256 * 8 ? nblk : 256 * 8), block(nw * kWave);
  // (an order whose chain has no term has no instantiation)
#define FIELD_CASE(PP) case PP: if constexpr (PP > Q::kDrop) hipLaunchKernelGGL((Q::template l2p_kernel<PP>()), grid, block, lds, s, d, p, n_src, tree); break;
  switch (p <= kUnrollMax ? p : 0) {
    FIELD_CASE(1) FIELD_CASE(2) FIELD_CASE(3) FIELD_CASE(4) FIELD_CASE(5) FIELD_CASE(6) FIELD_CASE(7) FIELD_CASE(8)
    FIELD_CASE(9) FIELD_CASE(10) FIELD_CASE(11) FIELD_CASE(12)
    default: hipLaunchKernelGGL((Q::template l2p_kernel<0>()), grid, block, lds, s, d, p, n_src, tree);
  }
#undef FIELD_CASE
  return hipGetLastError();
}

}  // namespace

hipError_t launch_near_field(FieldQuantity q, const DevicePlan& d, int64_t n_src, double* tree, hipStream_t s) {
  const int nleaf = d.leaf_end - d.leaf_begin;
  if (nleaf <= 0) return hipSuccess;
  return with_quantity(q, [&](auto Q) {
    using QT = decltype(Q);
    const int nblk = (nleaf + kNearWaves - 1) / kNearWaves, nf = QT::kRec + 3 * d.nq;
    const int pb = near_batch(nf);
    const size_t lds = sizeof(double) * (size_t)kNearWaves * pb * nf;
    hipLaunchKernelGGL(near_field_kernel<QT>, dim3(nblk < 256 * 16 ? nblk : 256 * 16), dim3(kNearWaves * kWave), lds, s, d, n_src, pb, tree);
    return hipGetLastError();
  });
}

// the pressure's and the velocity gradient's near pairs in one kernel (near_flow_kernel): the grid, the batch and the LDS of the
// velocity gradient's own launch
hipError_t launch_near_flow(const DevicePlan& d, int64_t n_src, double* q_tree, double* g_tree, hipStream_t s) {
  const int nleaf = d.leaf_end - d.leaf_begin;
  if (nleaf <= 0) return hipSuccess;
  const int nblk = (nleaf + kNearWaves - 1) / kNearWaves, nf = VelocityGradientQ::kRec + 3 * d.nq;
  const int pb = near_batch(nf);
  const size_t lds = sizeof(double) * (size_t)kNearWaves * pb * nf;
  hipLaunchKernelGGL(near_flow_kernel, dim3(nblk < 256 * 16 ? nblk : 256 * 16), dim3(kNearWaves * kWave), lds, s, d, n_src, pb, q_tree, g_tree);
  return hipGetLastError();
}

// both Laplace layers' near pairs, value and gradient, in one kernel (near_representation_kernel): sigma in d.xt, mu in mu_tree;
// a null tree buffer: that output is not computed
hipError_t launch_near_representation(const DevicePlan& d, int64_t n_src, const double* mu_tree, double* phi_tree, double* g_tree, hipStream_t s) {
  const int nleaf = d.leaf_end - d.leaf_begin;
  if (nleaf <= 0) return hipSuccess;
  if (!mu_tree || (!phi_tree && !g_tree)) return hipErrorInvalidValue;
  const int nblk = (nleaf + kNearWaves - 1) / kNearWaves, nf = kRepRec + 3 * d.nq;
  const int pb = representation_batch(nf);
  const size_t lds = sizeof(double) * (size_t)kNearWaves * pb * nf;
  const dim3 grid(nblk < 256 * 16 ? nblk : 256 * 16), block(kNearWaves * kWave);
  if (phi_tree && g_tree) hipLaunchKernelGGL((near_representation_kernel<true, true>), grid, block, lds, s, d, n_src, pb, mu_tree, phi_tree, g_tree);
  else if (phi_tree) hipLaunchKernelGGL((near_representation_kernel<true, false>), grid, block, lds, s, d, n_src, pb, mu_tree, phi_tree, g_tree);
  else hipLaunchKernelGGL((near_representation_kernel<false, true>), grid, block, lds, s, d, n_src, pb, mu_tree, phi_tree, g_tree);
  return hipGetLastError();
}

// M slot 0 += M slot 1 (set: =) at the P2M leaves, the coefficients of order p (fold_slots_kernel)
hipError_t launch_fold_slots(const DevicePlan& d, int p, bool set, hipStream_t s) {
  if (d.n_p2m <= 0) return hipSuccess;
  if (p < 1 || p > kPmaxDev || d.nslots != 2) return hipErrorInvalidValue;
  const int S = p * (p + 1) / 2;
  const int64_t n = (int64_t)d.n_p2m * S;
  hipLaunchKernelGGL(fold_slots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, S, set ? 1 : 0);
  return hipGetLastError();
}

// tree order -> distinct points for one double per row: the value of the representation execute
hipError_t launch_value_scatter(const DevicePlan& d, int64_t n_src, const double* tree, double* out, hipStream_t s) {
  const int64_t rows = d.n - n_src;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(field_scatter_kernel<1>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d.perm, tree, out, n_src, rows);
  return hipGetLastError();
}

hipError_t launch_l2p_field(FieldQuantity q, const DevicePlan& d, int p, int64_t n_src, double* tree, hipStream_t s) {
  if (d.n_l2p <= 0) return hipSuccess;
  return with_quantity(q, [&](auto Q) { return launch_l2p<decltype(Q)>(d, p, n_src, tree, s); });
}

hipError_t launch_field_scatter(FieldQuantity q, const DevicePlan& d, int64_t n_src, const double* tree, double* out, hipStream_t s) {
  const int64_t rows = d.n - n_src;
  if (rows <= 0) return hipSuccess;
  return with_quantity(q, [&](auto Q) {
    constexpr int W = decltype(Q)::kWidth;
    hipLaunchKernelGGL(field_scatter_kernel<W>, dim3((unsigned)((W * rows + 255) / 256)), dim3(256), 0, s, d.perm, tree, out, n_src, rows);
    return hipGetLastError();
  });
}

hipError_t launch_field_entries(FieldQuantity q, const DevicePlan& d, int m, double* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  const dim3 grid((m + 63) / 64), block(64);
  switch (q) {
    case FieldQuantity::Gradient: hipLaunchKernelGGL(grad_entries_kernel, grid, block, 0, s, d, m, out); break;
    case FieldQuantity::Pressure: hipLaunchKernelGGL(pressure_entries_kernel, grid, block, 0, s, d, m, out); break;
    case FieldQuantity::VelocityGradient: hipLaunchKernelGGL(velgrad_entries_kernel, grid, block, 0, s, d, m, out); break;
    case FieldQuantity::Hessian: hipLaunchKernelGGL(hess_entries_kernel, grid, block, 0, s, d, m, out); break;
  }
  return hipGetLastError();
}

}  // namespace fmmbem
