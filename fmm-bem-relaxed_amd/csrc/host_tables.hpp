// host_tables.hpp -- host-side tabulation shared by plan.hip (through plan_layout.hpp) and ops.hip, each table once: the
// EPS-scaled normalisation tables of the reference's spherical harmonics, cart2sph, the harmonics themselves, the step table, the
// class tables of the shifts and of M2L, the class record of the rotation kernels, and the tables of the order alone (OrderTables).
#pragma once
#include <cmath>
#include <complex>
#include <future>
#include <memory>
#include <mutex>
#include <vector>

#include "host_plan.hpp"
#include "m2l_layout.hpp"
#include "m2l_rot.hpp"
#include "shift_lanes.hpp"

namespace fmmbem {
namespace tables {

constexpr int kTabN = 2 * kPmax;        // harmonic degrees tabulated: n < 32
constexpr double kEps = 1e-12;          // kernel/LaplaceSpherical.hpp:30

// Anm / prefactor of LaplaceSpherical::precompute (kernel/LaplaceSpherical.hpp:87-104), for all degrees
// any p <= 16 needs.  The index n^2+n+m does not depend on P, so one table serves every order.
struct HarmonicTables {
  std::vector<double> A, invA, pref;
  HarmonicTables() : A(kTabN * kTabN), invA(kTabN * kTabN), pref(kTabN * kTabN) {
    for (int n = 0; n < kTabN; ++n)
      for (int m = -n; m <= n; ++m) {
        const int nm = n * n + n + m, am = std::abs(m);
        double fnmm = kEps, fnpm = kEps, fnma = 1.0, fnpa = 1.0;
        for (int i = 1; i <= n - m; ++i) fnmm *= i;
        for (int i = 1; i <= n + m; ++i) fnpm *= i;
        for (int i = 1; i <= n - am; ++i) fnma *= i;
        for (int i = 1; i <= n + am; ++i) fnpa *= i;
        pref[nm] = std::sqrt(fnma / fnpa);
        A[nm] = ((n & 1) ? -1.0 : 1.0) / std::sqrt(fnmm * fnpm);
        invA[nm] = 1.0 / A[nm];
      }
  }
};

struct SphHost { double rho, alpha, beta; };
// kernel/LaplaceSpherical.hpp:528-541
inline SphHost cart2sph_host(const double d[3]) {
  SphHost s;
  s.rho = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + kEps;
  s.alpha = std::acos(d[2] / s.rho);
  if (std::fabs(d[0]) + std::fabs(d[1]) < kEps) s.beta = 0;
  else if (std::fabs(d[0]) < kEps) s.beta = d[1] / std::fabs(d[1]) * M_PI * 0.5;
  else if (d[0] > 0) s.beta = std::atan(d[1] / d[0]);
  else s.beta = std::atan(d[1] / d[0]) + M_PI;
  return s;
}

using cplx = std::complex<double>;

// Harmonics for orders m >= 0, degrees n < N.  regular: rho^n P_n^m pref e^{i m beta}
// (evalMultipole, :455-488); otherwise rho^{-n-1} ... (evalLocal, :491-524).  out[n(n+1)/2+m].
inline void harmonics(const HarmonicTables& T, bool regular, double rho, double alpha, double beta, int N,
               std::vector<cplx>& out) {
  out.assign((size_t)N * (N + 1) / 2, cplx(0, 0));
  const double x = std::cos(alpha), y = std::sin(alpha);
  double fact = 1, pn = 1, rhom = regular ? 1.0 : 1.0 / rho;
  for (int m = 0; m < N; ++m) {
    const cplx eim = std::exp(cplx(0, 1) * double(m * beta));
    double p = pn;
    out[(size_t)m * (m + 1) / 2 + m] = rhom * p * T.pref[m * m + 2 * m] * eim;
    double p1 = p;
    p = x * (2 * m + 1) * p1;
    if (regular) rhom *= rho; else rhom /= rho;
    double rhon = rhom;
    for (int n = m + 1; n < N; ++n) {
      out[(size_t)n * (n + 1) / 2 + m] = rhon * p * T.pref[n * n + n + m] * eim;
      const double p2 = p1;
      p1 = p;
      p = (x * (2 * n + 1) * p1 - (n + m) * p2) / (n - m + 1);
      if (regular) rhon *= rho; else rhon /= rho;
    }
    pn = -pn * fact * y;
    fact += 2;
  }
}

inline cplx i_pow(int q) {
  switch (q & 3) { case 0: return {1, 0}; case 1: return {0, 1}; case 2: return {-1, 0}; default: return {0, -1}; }
}


// class record of the rotation kernels: 1/rho, cos alpha, sin alpha, cos beta, sin beta, rho of a translation vector --
// cart2sph of the reference (kernel/LaplaceSpherical.hpp:528-541): rho = |d| + EPS, alpha = acos(z / rho), and the azimuth
// branches; kept as cosines and sines
inline void rot_record(const double tr[3], double* o) {
  const double rho = std::sqrt(tr[0] * tr[0] + tr[1] * tr[1] + tr[2] * tr[2]) + kEps;
  const double ca = tr[2] / rho;
  o[0] = 1.0 / rho; o[1] = ca; o[2] = std::sqrt((1.0 - ca) * (1.0 + ca)); o[5] = rho; o[6] = o[7] = 0.0;
  if (std::fabs(tr[0]) + std::fabs(tr[1]) < kEps) { o[3] = 1; o[4] = 0; }
  else if (std::fabs(tr[0]) < kEps) { o[3] = 0; o[4] = tr[1] > 0 ? 1.0 : -1.0; }
  else { const double h = 1.0 / std::sqrt(tr[0] * tr[0] + tr[1] * tr[1]); o[3] = tr[0] * h; o[4] = tr[1] * h; }
}

// per-step constants of the harmonic recurrences in the m-major order P2M visits (n,m) at order p, {pref, c1, c2, 0} per
// (order, step): pref = sqrt((n-m)!/(n+m)!) and the Legendre step P_{n+1}^m = c1 x P_n^m - c2 P_{n-1}^m (c1 = 2m+1, c2 = 0 at n = m)
inline std::vector<double> step_table(const HarmonicTables& T) {
  const int smax = kPmax * (kPmax + 1) / 2;
  std::vector<double> st((size_t)kPmax * (smax + 1) * 4, 0.0);
  for (int p = 1; p <= kPmax; ++p) {
    double* o = st.data() + (size_t)(p - 1) * (smax + 1) * 4;
    for (int m = 0; m < p; ++m)
      for (int n = m; n < p; ++n, o += 4) {
        o[0] = T.pref[n * n + n + m];
        o[1] = n == m ? (double)(2 * m + 1) : (double)(2 * n + 1) * (1.0 / (n - m + 1));
        o[2] = n == m ? 0.0 : (double)(n + m) * (1.0 / (n - m + 1));
      }
  }
  return st;
}

// The [pm^2] table of one parent<->child translation class, appended to out: the regular harmonics of the translation for all
// (n, m), -n <= m <= n.  M2M: evalMultipole(rho, alpha, -beta) of (parent - child) (LaplaceSpherical.hpp:253-254); L2L:
// evalMultipole(rho, alpha, +beta) of (child - parent) (:383-384).  h: scratch.
inline void shift_class_table(const HarmonicTables& T, const double tr[3], bool m2m, int pm, std::vector<cplx>& h, std::vector<cplx>& out) {
  const SphHost s = cart2sph_host(tr);
  harmonics(T, true, s.rho, s.alpha, m2m ? -s.beta : s.beta, pm, h);
  for (int n = 0; n < pm; ++n)
    for (int m = -n; m <= n; ++m) {
      const cplx y = h[(size_t)n * (n + 1) / 2 + std::abs(m)];
      out.push_back(m < 0 ? std::conj(y) : y);
    }
}

// The rows of one M2L class (translation = c_target - c_source): Yh[r,c] = i^{|c|} EPS Y[r,c] / A[r,c] = Z^c gh[r,c], tabulated as
// the real part G (harmonics at beta = 0, evalLocal to order 2 pm; g[pm (2 pm + 1)]) and the phases Z^m = i^m e^{i m beta} (z[pm])
// separately (kernels_m2l.hip header).  h: scratch.
inline void m2l_class_rows(const HarmonicTables& T, const double tr[3], int pm, std::vector<cplx>& h, double* g, cplx* z) {
  const SphHost sp = cart2sph_host(tr);
  const int R = 2 * pm;
  harmonics(T, false, sp.rho, sp.alpha, 0.0, R, h);
  for (int r = 0; r < R; ++r)
    for (int cc = 0; cc <= r; ++cc)
      g[r * (r + 1) / 2 + cc] = h[(size_t)r * (r + 1) / 2 + cc].real() * kEps / T.A[r * r + r + cc];
  for (int m = 0; m < pm; ++m) z[m] = i_pow(m) * std::exp(cplx(0, 1) * double(m * sp.beta));
}

// Tables that depend on the expansion ORDER alone -- the constant streams of the three rotation kernels, the lanes' tables of the
// one-pair-per-wavefront shifts, the lane and scatter maps of the double-sum M2L: ~30 ms of host arithmetic that used to sit on
// every plan's critical path.  Built once per process, on a thread of their own that the first caller of order_tables() starts
// (fmmbem_plan_create calls it BEFORE it builds the tree); whoever uploads them waits for them there.
struct OrderTables {
  std::vector<double> rot_all, ups, dns;
  int rot_off[kRotPmax] = {}, shift_off[kRotPmax] = {};
  std::vector<double> urc, uxc, drc, dxc;
  std::vector<int32_t> urs, uxs, drs, dxs;
  size_t sl_rot_off[kShiftLanesPmax + 1] = {}, sl_ax_off[kShiftLanesPmax + 1] = {};
  std::vector<int32_t> lanes, scat;
  int scat_off[kPmax] = {};
  bool lanes_ok = true;
};
inline std::shared_ptr<const OrderTables> build_order_tables() {
  auto t = std::make_shared<OrderTables>();
  std::vector<double> one;
  for (int q = 1; q <= kRotPmax; ++q) {
    t->rot_off[q - 1] = (int)t->rot_all.size();
    build_rot_stream(q, one); t->rot_all.insert(t->rot_all.end(), one.begin(), one.end());
    t->shift_off[q - 1] = (int)t->ups.size();
    build_rot_stream(q, one, kRotM2M); t->ups.insert(t->ups.end(), one.begin(), one.end());
    // both shifts have the same number of axial terms: one offset table serves the two streams
    build_rot_stream(q, one, kRotL2L); t->dns.insert(t->dns.end(), one.begin(), one.end());
  }
  ShiftLaneTables lt;
  for (int q = 1; q <= kShiftLanesPmax; ++q) {
    t->sl_rot_off[q] = t->urc.size(); t->sl_ax_off[q] = t->uxc.size();
    build_shift_lane_tables(q, kRotM2M, lt);
    t->urc.insert(t->urc.end(), lt.rot_c.begin(), lt.rot_c.end()); t->urs.insert(t->urs.end(), lt.rot_s.begin(), lt.rot_s.end());
    t->uxc.insert(t->uxc.end(), lt.ax_c.begin(), lt.ax_c.end()); t->uxs.insert(t->uxs.end(), lt.ax_s.begin(), lt.ax_s.end());
    build_shift_lane_tables(q, kRotL2L, lt);
    t->drc.insert(t->drc.end(), lt.rot_c.begin(), lt.rot_c.end()); t->drs.insert(t->drs.end(), lt.rot_s.begin(), lt.rot_s.end());
    t->dxc.insert(t->dxc.end(), lt.ax_c.begin(), lt.ax_c.end()); t->dxs.insert(t->dxs.end(), lt.ax_s.begin(), lt.ax_s.end());
  }
  std::vector<int32_t> m;
  for (int p = 1; p <= kPmax; ++p) {
    if (!m2l_lane_map(p, m)) t->lanes_ok = false;
    t->lanes.insert(t->lanes.end(), m.begin(), m.end());
    m2l_scatter_map(p, m);
    t->scat_off[p - 1] = (int)t->scat.size();
    t->scat.insert(t->scat.end(), m.begin(), m.end());
  }
  return t;
}
inline std::shared_future<std::shared_ptr<const OrderTables>> order_tables() {
  static std::mutex mu;
  static std::shared_future<std::shared_ptr<const OrderTables>> fut;
  std::lock_guard<std::mutex> lock(mu);
  if (!fut.valid()) fut = std::async(std::launch::async, build_order_tables).share();
  return fut;
}

}  // namespace tables
}  // namespace fmmbem
