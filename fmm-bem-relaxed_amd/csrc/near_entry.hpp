// near_entry.hpp -- one entry of the operator: K(target point, source panel j) of a DevicePlan's panels, in every regime.
// laplace_entry / stokes_entry are the ONE text of that arithmetic; the near-matrix assembly, the matrix-free passes and
// fmmbem_kernel_entries (kernels_near.hip) and the Direct sum (kernels_direct.hip) all call it, so that an entry's bits do not
// depend on who asks.
#pragma once
#include "device_plan.hpp"

namespace fmmbem {

namespace {

struct V3 { double x, y, z; };
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 cross(V3 u, V3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ inline double norm(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ inline V3 mul3(const double* M, V3 v) {       // row-major 3x3 times vector (include/Mat3.hpp:76-82)
  return {M[0] * v.x + M[1] * v.y + M[2] * v.z, M[3] * v.x + M[4] * v.y + M[5] * v.z, M[6] * v.x + M[7] * v.y + M[8] * v.z};
}

// 5-point Gauss-Legendre in the polar angle along one triangle edge
// (examples/BEM/SemiAnalytical.hpp:13-71, LAPLACE branch; only G is needed by the Laplace near field)
__device__ inline double edge_angle_integral(double z, double x, double v1, double v2) {
  const double t1 = atan2(v1, x), t2 = atan2(v2, x);
  const double dt = t2 - t1, tm = (t2 + t1) / 2;
  const double az = fabs(z);
  const double xk[5] = {-9.06179846e-01, -5.38469310e-01, 1.78162900e-17, 9.06179846e-01, 5.38469310e-01};
  const double wk[5] = {0.23692689, 0.47862867, 0.56888889, 0.23692689, 0.47862867};
  double G = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double tk = dt / 2 * xk[i] + tm;
    const double Rt = x / cos(tk);
    const double R = sqrt(Rt * Rt + z * z);
    G += wk[i] * (R - az) * dt / 2;
  }
  return G;
}

// contribution of one edge v1->v2, in the panel plane with the collocation point at the origin and
// height p above the plane (examples/BEM/SemiAnalytical.hpp:81-145)
__device__ inline double edge_term(V3 v1, V3 v2, double p) {
  const V3 e = sub(v2, v1);
  const double len = norm(e);
  const V3 u = {e.x / len, e.y / len, e.z / len};
  const V3 o = cross(V3{0, 0, 1}, u);
  double R[9] = {o.x, u.x, 0, o.y, u.y, 0, o.z, u.z, 1};
  V3 a = mul3(R, v1);
  if (a.x < 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = -R[i];
    R[8] = 1.;
    a = mul3(R, v1);
  }
  const V3 b = mul3(R, v2);
  if ((a.y > 0 && b.y < 0) || (a.y < 0 && b.y > 0))
    return edge_angle_integral(p, a.x, 0, a.y) + edge_angle_integral(p, a.x, b.y, 0);
  return -edge_angle_integral(p, a.x, a.y, b.y);
}

// int_panel 1/|x - y| dS(y), semi-analytically (examples/BEM/SemiAnalytical.hpp:148-203)
__device__ inline double semi_analytic_G(V3 y0, V3 y1, V3 y2, V3 x) {
  const V3 xp = sub(x, y0), e1 = sub(y1, y0), e2 = sub(y2, y0);
  V3 X = e1, Z = cross(e1, e2);
  const double xn = norm(X), zn = norm(Z);
  X = {X.x / xn, X.y / xn, X.z / xn};
  Z = {Z.x / zn, Z.y / zn, Z.z / zn};
  const V3 Y = cross(Z, X);
  const double rot[9] = {X.x, X.y, X.z, Y.x, Y.y, Y.z, Z.x, Z.y, Z.z};
  const V3 q0 = mul3(rot, V3{0, 0, 0}), q1 = mul3(rot, e1), q2 = mul3(rot, e2), xq = mul3(rot, xp);
  const V3 f0 = {q0.x - xq.x, q0.y - xq.y, q0.z}, f1 = {q1.x - xq.x, q1.y - xq.y, q1.z}, f2 = {q2.x - xq.x, q2.y - xq.y, q2.z};
  return edge_term(f0, f1, xq.z) + edge_term(f1, f2, xq.z) + edge_term(f2, f0, xq.z);
}

// the 16-point "K_fine" rule keyed 17 (examples/BEM/GaussQuadrature.hpp:86-116), barycentric
__constant__ double kFine[16][4] = {
    {1. / 3, 1. / 3, 1. / 3, 0.144315607677787},
    {0.081414823414554, 0.459292588292723, 0.459292588292723, 0.095091634267285},
    {0.459292588292723, 0.081414823414554, 0.459292588292723, 0.095091634267285},
    {0.459292588292723, 0.459292588292723, 0.081414823414554, 0.095091634267285},
    {0.658861384496480, 0.170569307751760, 0.170569307751760, 0.103217370534718},
    {0.170569307751760, 0.658861384496480, 0.170569307751760, 0.103217370534718},
    {0.170569307751760, 0.170569307751760, 0.658861384496480, 0.103217370534718},
    {0.898905543365938, 0.050547228317031, 0.050547228317031, 0.032458497623198},
    {0.050547228317031, 0.898905543365938, 0.050547228317031, 0.032458497623198},
    {0.050547228317031, 0.050547228317031, 0.898905543365938, 0.032458497623198},
    {0.008394777409958, 0.263112829634638, 0.728492392955404, 0.027230314174435},
    {0.008394777409958, 0.728492392955404, 0.263112829634638, 0.027230314174435},
    {0.263112829634638, 0.008394777409958, 0.728492392955404, 0.027230314174435},
    {0.263112829634638, 0.728492392955404, 0.008394777409958, 0.027230314174435},
    {0.728492392955404, 0.008394777409958, 0.263112829634638, 0.027230314174435},
    {0.728492392955404, 0.263112829634638, 0.008394777409958, 0.027230314174435}};

// One near-matrix entry: target centroid t with BC flag, source panel j (tree index).
// kernel/LaplaceSphericalBEM.hpp:273-297 -> eval_G (:159-205) / eval_dGdn (:208-264)
// In two parts, so that the assembly can run the expensive regime with full wavefronts: laplace_entry_far gives the entry of a
// pair in the far regime (the K stored Gauss points; also the 2 pi of a NORMAL_DERIV self pair) or says `deferred`;
// laplace_entry_near gives the near regime (semi-analytic G, :166-178; the 16-point rule for dG/dn, :222-243).
// the far regime's arithmetic on a source panel held in registers (one text for both callers: the bits must not depend on who asks)
template <class Quad>
__device__ __forceinline__ double laplace_far_from(V3 t, int tbc, V3 c, double A, V3 nrm, int nq, const double* qw, Quad&& quad, bool& deferred) {
  const double dist = norm(sub(t, c));
  const bool nearby = sqrt(2 * A) / dist >= 0.5;
  deferred = false;
  if (tbc == 0) {                                   // POTENTIAL target: int G
    if (nearby) { deferred = true; return 0; }
    double r = 0;
    for (int q = 0; q < nq; ++q) {
      const V3 qp = quad(q);
      r += qw[q] * A / norm(sub(t, qp));
    }
    return r;
  }
  // NORMAL_DERIV target: int dG/dn
  if (dist < 1e-8) return 2 * M_PI;
  if (nearby) { deferred = true; return 0; }
  double r = 0;
  for (int q = 0; q < nq; ++q) {
    const V3 qp = quad(q);
    const V3 dx = sub(qp, t);
    const double r2 = dx.x * dx.x + dx.y * dx.y + dx.z * dx.z;
    r += qw[q] * A * (dx.x * nrm.x + dx.y * nrm.y + dx.z * nrm.z) / (r2 * sqrt(r2));
  }
  return r;
}
__device__ inline double laplace_entry_far(const DevicePlan& d, V3 t, int tbc, int64_t j, bool& deferred) {
  const int64_t N = d.n;
  const V3 c = {d.cx[j], d.cy[j], d.cz[j]};
  const V3 nrm = tbc ? V3{d.nx[j], d.ny[j], d.nz[j]} : V3{0, 0, 0};
  return laplace_far_from(t, tbc, c, d.area[j], nrm, d.nq, d.qw,
                          [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; }, deferred);
}
__device__ inline double laplace_entry_near(const DevicePlan& d, V3 t, int tbc, int64_t j) {
  const int64_t N = d.n;
  const V3 v0 = {d.vert[0 * N + j], d.vert[1 * N + j], d.vert[2 * N + j]};
  const V3 v1 = {d.vert[3 * N + j], d.vert[4 * N + j], d.vert[5 * N + j]};
  const V3 v2 = {d.vert[6 * N + j], d.vert[7 * N + j], d.vert[8 * N + j]};
  if (tbc == 0) return semi_analytic_G(v0, v1, v2, t);
  const double A = d.area[j];
  const V3 nrm = {d.nx[j], d.ny[j], d.nz[j]};
  double r = 0;
  for (int q = 0; q < 16; ++q) {
    const V3 pt = {v0.x * kFine[q][0] + v1.x * kFine[q][1] + v2.x * kFine[q][2],
                   v0.y * kFine[q][0] + v1.y * kFine[q][1] + v2.y * kFine[q][2],
                   v0.z * kFine[q][0] + v1.z * kFine[q][1] + v2.z * kFine[q][2]};
    const V3 dx = sub(pt, t);
    const double r2 = dx.x * dx.x + dx.y * dx.y + dx.z * dx.z;
    r += kFine[q][3] * A * (dx.x * nrm.x + dx.y * nrm.y + dx.z * nrm.z) / (r2 * sqrt(r2));
  }
  return r;
}
__device__ inline double laplace_entry(const DevicePlan& d, V3 t, int tbc, int64_t j) {
  bool deferred;
  const double v = laplace_entry_far(d, t, tbc, j, deferred);
  return deferred ? laplace_entry_near(d, t, tbc, j) : v;
}

// The gradient, with respect to the target point t, of the integrand the target's flag picks (include/fmmbem.h, "Field gradient"):
// three doubles per (target point, source panel j).  The regimes are those of a NORMAL_DERIV target above: self (dist < 1e-8),
// nearby (the 16-point rule on the vertices), else the K stored points; points in order, one running sum.  With dx = y_q - t:
//   flag 0 (single layer, int G):        sum_q w_q A dx / |dx|^3;                                self: 2 pi n_j
//   flag 1 (double layer, int dG/dn_y):  sum_q w_q A (-n_j / |dx|^3 + 3 (dx . n_j) dx / |dx|^5);  self: 0
// so n_j . (flag 0) is the NORMAL_DERIV entry of the pair.  The ONE text of it: the matrix-free near kernel of the gradient execute
// and fmmbem_kernel_gradient_entries (kernels_grad.hip) both call it: laplace_grad_from on a panel's fields, laplace_grad_entry on panel j of d.
// (the arithmetic on a source panel handed over by its fields: quad(q) the stored point q, vert(a) vertex a, read only in the near regime)
template <class Quad, class Vert>
__device__ __forceinline__ V3 laplace_grad_from(V3 t, int tbc, V3 c, double A, V3 nrm, int nq, const double* qw, Quad&& quad, Vert&& vert) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  // The regime is decided by the expressions of laplace_far_from, dist < 1e-8 and sqrt(2 A) / dist >= 0.5, so that a pair is in the
  // same regime there and here.  Most pairs are far from that boundary: with 8 A < 0.99 dist^2 the exact ratio is below 0.4975 and
  // its few roundings cannot lift it to 0.5 (and dist^2 > 1e-15 is no self pair), so the square root and the division are skipped.
  bool nearby = false;
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {
    const double dist = sqrt(d2);
    if (dist < 1e-8) {
      const double s = tbc ? 0.0 : 2 * M_PI;
      return {s * nrm.x, s * nrm.y, s * nrm.z};
    }
    nearby = sqrt(2 * A) / dist >= 0.5;
  }
  V3 g = {0, 0, 0};
  auto point = [&](V3 y, double wA) {
    const V3 dx = sub(y, t);
    const double r2 = dx.x * dx.x + dx.y * dx.y + dx.z * dx.z;
    const double ri = rsqrt(r2), ri2 = ri * ri;          // 1 / |dx|: one reciprocal square root per point, no division
    const double f = wA * (ri * ri2);
    if (tbc == 0) {
      g.x += f * dx.x; g.y += f * dx.y; g.z += f * dx.z;
    } else {
      const double h = 3 * (dx.x * nrm.x + dx.y * nrm.y + dx.z * nrm.z) * ri2;
      g.x += f * (h * dx.x - nrm.x); g.y += f * (h * dx.y - nrm.y); g.z += f * (h * dx.z - nrm.z);
    }
  };
  if (nearby) {
    const V3 v0 = vert(0), v1 = vert(1), v2 = vert(2);
    for (int q = 0; q < 16; ++q)
      point(V3{v0.x * kFine[q][0] + v1.x * kFine[q][1] + v2.x * kFine[q][2], v0.y * kFine[q][0] + v1.y * kFine[q][1] + v2.y * kFine[q][2],
               v0.z * kFine[q][0] + v1.z * kFine[q][1] + v2.z * kFine[q][2]}, kFine[q][3] * A);
  } else {
    for (int q = 0; q < nq; ++q) point(quad(q), qw[q] * A);
  }
  return g;
}
__device__ inline V3 laplace_grad_entry(const DevicePlan& d, V3 t, int tbc, int64_t j) {
  const int64_t N = d.n;
  return laplace_grad_from(t, tbc, V3{d.cx[j], d.cy[j], d.cz[j]}, d.area[j], V3{d.nx[j], d.ny[j], d.nz[j]}, d.nq, d.qw,
                           [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; },
                           [&](int a) { return V3{d.vert[(3 * a + 0) * N + j], d.vert[(3 * a + 1) * N + j], d.vert[(3 * a + 2) * N + j]}; });
}

// The Hessian: the derivative, with respect to the target point t, of the gradient above (include/fmmbem.h, "Field Hessian"): a
// symmetric, trace-free 3x3 per (target point, source panel j), held as its upper triangle xx, xy, xz, yy, yz, zz.  The regime is
// decided by laplace_grad_from's expressions, shortcut included, so that a pair is in the same regime there and here; a self pair
// (dist < 1e-8) gives 0 for both flags.  With dx = y_q - t, r = |dx|, n the panel normal:
//   flag 0:  sum_q w_q A (3 dx_a dx_b / r^5 - delta_ab / r^3)
//   flag 1:  sum_q w_q A (15 (dx.n) dx_a dx_b / r^7 - 3 (n_a dx_b + n_b dx_a + (dx.n) delta_ab) / r^5)
// One reciprocal square root per point, no division; points in order, one running sum per component.  The ONE text of it: the near
// kernel of the Hessian execute, fmmbem_kernel_hessian_entries and the Direct sum call it: laplace_hess_from adds x times the pair to
// six sums (x = 1 from zero sums: the entry), laplace_hess_entry is the entry of panel j of d.
struct Sym3 { double xx, xy, xz, yy, yz, zz; };
template <class Quad, class Vert>
__device__ __forceinline__ void laplace_hess_from(V3 t, int tbc, V3 c, double A, V3 nrm, int nq, const double* qw, Quad&& quad, Vert&& vert,
                                                  double x, Sym3& acc) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  bool nearby = false;
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {              // (see laplace_grad_from: far from the regime boundary, no square root)
    const double dist = sqrt(d2);
    if (dist < 1e-8) return;
    nearby = sqrt(2 * A) / dist >= 0.5;
  }
  // From here on nothing is left to the compiler's contraction: every fused multiply-add is written, so that the entry has the
  // same bits in every kernel that asks for it.
  {
#pragma clang fp contract(off)
    Sym3 h = {0, 0, 0, 0, 0, 0};
    auto point = [&](V3 y, double wA) {
#pragma clang fp contract(off)
      const V3 dx = sub(y, t);
      const double r2 = __builtin_fma(dx.z, dx.z, __builtin_fma(dx.y, dx.y, dx.x * dx.x));
      const double ri = rsqrt(r2), ri2 = ri * ri;        // 1 / |dx|: one reciprocal square root per point, no division
      const double f3 = wA * (ri * ri2), f5 = 3 * f3 * ri2;
      if (tbc == 0) {
        const V3 u = {f5 * dx.x, f5 * dx.y, f5 * dx.z};
        h.xx = __builtin_fma(u.x, dx.x, h.xx - f3); h.xy = __builtin_fma(u.x, dx.y, h.xy); h.xz = __builtin_fma(u.x, dx.z, h.xz);
        h.yy = __builtin_fma(u.y, dx.y, h.yy - f3); h.yz = __builtin_fma(u.y, dx.z, h.yz);
        h.zz = __builtin_fma(u.z, dx.z, h.zz - f3);
      } else {
        const double dn = __builtin_fma(dx.z, nrm.z, __builtin_fma(dx.y, nrm.y, dx.x * nrm.x));
        const double s = f5 * dn, g = (5 * ri2) * s;     // 3 (dx.n) / r^5 and 15 (dx.n) / r^7, times wA
        const V3 u = {g * dx.x, g * dx.y, g * dx.z}, v = {-f5 * nrm.x, -f5 * nrm.y, -f5 * nrm.z};
        h.xx = __builtin_fma(u.x, dx.x, __builtin_fma(v.x + v.x, dx.x, h.xx - s));
        h.xy = __builtin_fma(u.x, dx.y, __builtin_fma(v.x, dx.y, __builtin_fma(v.y, dx.x, h.xy)));
        h.xz = __builtin_fma(u.x, dx.z, __builtin_fma(v.x, dx.z, __builtin_fma(v.z, dx.x, h.xz)));
        h.yy = __builtin_fma(u.y, dx.y, __builtin_fma(v.y + v.y, dx.y, h.yy - s));
        h.yz = __builtin_fma(u.y, dx.z, __builtin_fma(v.y, dx.z, __builtin_fma(v.z, dx.y, h.yz)));
        h.zz = __builtin_fma(u.z, dx.z, __builtin_fma(v.z + v.z, dx.z, h.zz - s));
      }
    };
    if (nearby) {
      const V3 v0 = vert(0), v1 = vert(1), v2 = vert(2);
      for (int q = 0; q < 16; ++q)
        point(V3{v0.x * kFine[q][0] + v1.x * kFine[q][1] + v2.x * kFine[q][2], v0.y * kFine[q][0] + v1.y * kFine[q][1] + v2.y * kFine[q][2],
                 v0.z * kFine[q][0] + v1.z * kFine[q][1] + v2.z * kFine[q][2]}, kFine[q][3] * A);
    } else {
      for (int q = 0; q < nq; ++q) point(quad(q), qw[q] * A);
    }
    // the pair's eta is rounded before the charge meets it, whoever asks: fma(eta_c, x, acc_c)
    acc.xx = __builtin_fma(h.xx, x, acc.xx); acc.xy = __builtin_fma(h.xy, x, acc.xy); acc.xz = __builtin_fma(h.xz, x, acc.xz);
    acc.yy = __builtin_fma(h.yy, x, acc.yy); acc.yz = __builtin_fma(h.yz, x, acc.yz); acc.zz = __builtin_fma(h.zz, x, acc.zz);
  }
}
__device__ inline void laplace_hess_entry(const DevicePlan& d, V3 t, int tbc, int64_t j, double x, Sym3& acc) {
  const int64_t N = d.n;
  laplace_hess_from(t, tbc, V3{d.cx[j], d.cy[j], d.cz[j]}, d.area[j], V3{d.nx[j], d.ny[j], d.nz[j]}, d.nq, d.qw,
                    [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; },
                    [&](int a) { return V3{d.vert[(3 * a + 0) * N + j], d.vert[(3 * a + 1) * N + j], d.vert[(3 * a + 2) * N + j]}; }, x, acc);
}

// Both layers of one pair TOGETHER, value and gradient (include/fmmbem.h, "Representation execute"): what panel j with density
// sigma and surface potential mu adds to   phi = sum E0 sigma - E1 mu   and   grad = sum gamma0 sigma - gamma1 mu   at the point t,
// E0 / E1 the entries of a flag-0 / flag-1 target above and gamma0 / gamma1 the two gradients of laplace_grad_from.  ONE regime test
// -- laplace_grad_from's expressions, which are laplace_far_from's -- and per quadrature point one dx = y_q - t, |dx|^2 and
// reciprocal square root feeding all four integrands, the densities folded in at the point:
//   phi  += wA ri sigma  -  wA ri^3 (dx . n) mu
//   grad += wA ri^3 dx sigma  -  wA ri^3 (h dx - n) mu  =  wA ri^3 ((sigma - h mu) dx + mu n),      h = 3 (dx . n) ri^2
// The regimes: self (dist < 1e-8): E0 semi-analytic (a flag-0 target has no self test and is nearby there), E1 = 2 pi,
// gamma0 = 2 pi n, gamma1 = 0; nearby: the 16-point rule on the vertices for E1, gamma0 and gamma1 in one loop and semi_analytic_G
// beside it for E0; else the K stored points for all four.  VALUE / GRAD: which of the two sums are kept (the other's
// arithmetic is compiled out).  Points in order, one running sum each: the same bits every run.
template <bool VALUE, bool GRAD, class Quad, class Vert>
__device__ __forceinline__ void laplace_representation_from(V3 t, V3 c, double A, V3 nrm, double sigma, double mu, int nq, const double* qw,
                                                            Quad&& quad, Vert&& vert, double& phi, V3& g) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  bool nearby = false, self = false;
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {              // (see laplace_grad_from: far from the regime boundary, no square root)
    const double dist = sqrt(d2);
    self = dist < 1e-8;
    nearby = self || sqrt(2 * A) / dist >= 0.5;
  }
  const V3 mn = {mu * nrm.x, mu * nrm.y, mu * nrm.z};
  auto point = [&](V3 y, double wA, bool with_e0) {
    const V3 dx = sub(y, t);
    const double r2 = dx.x * dx.x + dx.y * dx.y + dx.z * dx.z;
    const double ri = rsqrt(r2), ri2 = ri * ri;
    const double f = wA * (ri * ri2);
    const double dn = dx.x * nrm.x + dx.y * nrm.y + dx.z * nrm.z;
    if (VALUE) {
      phi -= f * dn * mu;
      if (with_e0) phi += wA * ri * sigma;
    }
    if (GRAD) {
      const double a = sigma - 3 * dn * ri2 * mu;
      g.x += f * (a * dx.x + mn.x); g.y += f * (a * dx.y + mn.y); g.z += f * (a * dx.z + mn.z);
    }
  };
  if (nearby) {
    const V3 v0 = vert(0), v1 = vert(1), v2 = vert(2);
    if (self) {
      if (VALUE) phi -= 2 * M_PI * mu;
      if (GRAD) {
        const double s = 2 * M_PI * sigma;
        g.x += s * nrm.x; g.y += s * nrm.y; g.z += s * nrm.z;
      }
    } else {
      for (int q = 0; q < 16; ++q)
        point(V3{v0.x * kFine[q][0] + v1.x * kFine[q][1] + v2.x * kFine[q][2], v0.y * kFine[q][0] + v1.y * kFine[q][1] + v2.y * kFine[q][2],
                 v0.z * kFine[q][0] + v1.z * kFine[q][1] + v2.z * kFine[q][2]}, kFine[q][3] * A, false);
    }
    // (one call for both regimes, and last: while it runs the pair's normal, area and weights are dead)
    if (VALUE) phi += semi_analytic_G(v0, v1, v2, t) * sigma;
  } else {
    for (int q = 0; q < nq; ++q) point(quad(q), qw[q] * A, true);
  }
}

// ---------------------------------------------------------------------------------------------
// Stokes (velocity boundary condition): one near-matrix entry is the 3x3 block
//   (1/2mu) int_source ( I/r + d d^T / r^3 ) dS,  d = target centroid - y
// (kernel/StokesSphericalBEM.hpp:260-375).  Regimes: far -> the K stored Gauss points (:352-369);
// near (sqrt(2A)/dist >= 0.5) -> the K_fine rule on the vertices (:302-321); self -> Fata's closed form.
// ---------------------------------------------------------------------------------------------
__device__ inline void stokeslet_point(double* res, double wA, V3 t, V3 pnt) {
  const V3 dd = sub(t, pnt);
  const double r2 = dd.x * dd.x + dd.y * dd.y + dd.z * dd.z;
  double invR2 = 1. / r2;
  if (r2 < 1e-8) invR2 = 0;
  const double f = wA * invR2 * sqrt(invR2);
  const double dv[3] = {dd.x, dd.y, dd.z};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) res[3 * i + j] += f * ((i == j ? r2 : 0.0) + dv[i] * dv[j]);
}

// Self term: AnalyticalIntegral::FataAnalytical<STOKES>(y1,y2,y3,.,x = centroid, self = true, G)
// (examples/BEM/FataAnalytical.hpp:414-690, self branch :535-539) + Integration<STOKES>::integrate (:273-341).
// With the collocation point in the panel plane (et = 0) and chi left at {0,0,0} in the self branch, only
// omega (three logarithms) and the rho-difference terms survive.
__device__ inline void stokes_self(V3 y1, V3 y2, V3 y3, V3 x, double* IU) {
  const double pi = M_PI;
  const V3 v1 = sub(y2, y1), v3 = sub(y3, y1);
  const double snrm = v1.x * v1.x + v1.y * v1.y + v1.z * v1.z, nrm = sqrt(snrm);
  const double al = (v1.x * v3.x + v1.y * v3.y + v1.z * v3.z) / snrm;
  V3 e2 = {v3.x - al * v1.x, v3.y - al * v1.y, v3.z - al * v1.z};
  const double nrx = norm(e2);
  const V3 e1 = {v1.x / nrm, v1.y / nrm, v1.z / nrm};
  e2 = {e2.x / nrx, e2.y / nrx, e2.z / nrx};
  const V3 e3 = {e1.y * e2.z - e2.y * e1.z, e1.z * e2.x - e2.z * e1.x, e1.x * e2.y - e2.x * e1.y};
  const double bQ = v1.x * e1.x + v1.y * e1.y + v1.z * e1.z;
  const double aQ = v3.x * e2.x + v3.y * e2.y + v3.z * e2.z;
  const double cQ = v3.x * e1.x + v3.y * e1.y + v3.z * e1.z;
  const double bmc = bQ - cQ, aQs = aQ * aQ;
  const double th0 = acos(cQ / sqrt(cQ * cQ + aQs)), th1 = acos(bmc / sqrt(bmc * bmc + aQs));
  const double alpha2 = pi - th1, alpha3 = pi + th0;
  const double cs2 = cos(alpha2), sn2 = sin(alpha2), cs3 = cos(alpha3), sn3 = sin(alpha3);
  const V3 r1 = sub(x, y1);
  const double xi = r1.x * e1.x + r1.y * e1.y + r1.z * e1.z;
  const double zt = r1.x * e2.x + r1.y * e2.y + r1.z * e2.z;
  double q[3];
  const double p11 = -xi, p12 = bQ - xi;
  q[0] = -zt;
  const double x3 = cQ + p11, z3 = aQ + q[0];
  const double p22 = p12 * cs2 + q[0] * sn2, p23 = x3 * cs2 + z3 * sn2;
  q[1] = q[0] * cs2 - p12 * sn2;
  const double p31 = p11 * cs3 + q[0] * sn3, p33 = x3 * cs3 + z3 * sn3;
  q[2] = q[0] * cs3 - p11 * sn3;
  const double rho[3] = {sqrt(p11 * p11 + q[0] * q[0]), sqrt(p12 * p12 + q[0] * q[0]), sqrt(p33 * p33 + q[2] * q[2])};
  const double omega = q[0] * log((p11 + rho[0]) / (p12 + rho[1])) + q[1] * log((p22 + rho[1]) / (p23 + rho[2])) +
                       q[2] * log((p33 + rho[2]) / (p31 + rho[0]));
  const double alpha[3] = {0., alpha2, alpha3};
  const double rb[3] = {rho[0] - rho[1], rho[1] - rho[2], rho[2] - rho[0]};
  double Ixx = 0, Izz = 0, Izx = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Ixx += (rb[i] * sin(alpha[i])) * cos(alpha[i]);
    Izz += (-rb[i] * cos(alpha[i])) * sin(alpha[i]);
    Izx += (rb[i] * sin(alpha[i])) * sin(alpha[i]);
  }
  const double E[3][3] = {{e1.x, e1.y, e1.z}, {e2.x, e2.y, e2.z}, {e3.x, e3.y, e3.z}};
  const double coef[3][3] = {{omega + Ixx, Izx, 0.0}, {Izx, omega + Izz, 0.0}, {0.0, 0.0, omega}};
#pragma unroll
  for (int i = 0; i < 9; ++i) IU[i] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) IU[3 * i + j] += coef[a][b] * E[a][i] * E[b][j];
}

// one Gauss point of the traction (double-layer) integrand: res += w A (d . n) d d^T / r^5, d = target - point
// (kernel/StokesSphericalBEM.hpp:205-225, 236-252)
__device__ inline void stresslet_point(double* res, double wA, V3 t, V3 pnt, V3 nrm) {
  const V3 dd = sub(t, pnt);
  const double r2 = dd.x * dd.x + dd.y * dd.y + dd.z * dd.z;
  double invR2 = 1. / r2;
  if (r2 < 1e-8) invR2 = 0;
  const double invR5 = invR2 * invR2 * sqrt(invR2);
  const double dn = dd.x * nrm.x + dd.y * nrm.y + dd.z * nrm.z;
  const double f = wA * dn * invR5;
  const double dv[3] = {dd.x, dd.y, dd.z};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) res[3 * i + j] += f * dv[i] * dv[j];
}

// tbc = the TARGET's flag (kernel/StokesSphericalBEM.hpp:377-389): 0 VELOCITY -> eval_velocity_integral (:260-375),
// 1 TRACTION -> eval_traction_integral (:160-258): self 2 pi I, near K_fine, far K points, times -3, no 1/(2 mu)
// In two parts like laplace_entry: stokes_far_from gives the block of a pair in the far regime (the K stored Gauss points; the
// 2 pi I of a TRACTION self pair) from a source panel held in registers, or says `deferred`; stokes_entry_near the near regime
// (the K_fine rule on the vertices, the closed form of the self pair).  One text for the arithmetic, whoever asks.
template <class Quad>
__device__ __forceinline__ bool stokes_far_from(const DevicePlan& d, V3 t, int tbc, V3 c, double A, V3 nrm, Quad&& quad, double* out) {
  const double dist = norm(sub(t, c));
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = 0;
  if (tbc) {
    if (fabs(dist) < 1e-8) { out[0] = out[4] = out[8] = 2 * M_PI; return false; }
    if (sqrt(2 * A) / dist >= 0.5) return true;
    for (int q = 0; q < d.nq; ++q) stresslet_point(out, d.qw[q] * A, t, quad(q), nrm);
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] *= -3.;
    return false;
  }
  if (sqrt(2 * A) / dist >= 0.5) return true;
  for (int q = 0; q < d.nq; ++q) stokeslet_point(out, d.qw[q] * A, t, quad(q));
  const double sc = 1. / 2 / d.mu;
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] *= sc;
  return false;
}
__device__ inline void stokes_entry_near(const DevicePlan& d, V3 t, int tbc, int64_t j, double* out) {
  const int64_t N = d.n;
  const V3 c = {d.cx[j], d.cy[j], d.cz[j]};
  const double A = d.area[j];
  const double dist = norm(sub(t, c));
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = 0;
  const V3 v0 = {d.vert[0 * N + j], d.vert[1 * N + j], d.vert[2 * N + j]};
  const V3 v1 = {d.vert[3 * N + j], d.vert[4 * N + j], d.vert[5 * N + j]};
  const V3 v2 = {d.vert[6 * N + j], d.vert[7 * N + j], d.vert[8 * N + j]};
  if (tbc) {
    const V3 nrm = {d.nx[j], d.ny[j], d.nz[j]};
    for (int q = 0; q < d.nqf; ++q) {
      const V3 pt = {v0.x * d.qf[4 * q + 0] + v1.x * d.qf[4 * q + 1] + v2.x * d.qf[4 * q + 2],
                     v0.y * d.qf[4 * q + 0] + v1.y * d.qf[4 * q + 1] + v2.y * d.qf[4 * q + 2],
                     v0.z * d.qf[4 * q + 0] + v1.z * d.qf[4 * q + 1] + v2.z * d.qf[4 * q + 2]};
      stresslet_point(out, d.qf[4 * q + 3] * A, t, pt, nrm);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] *= -3.;
    return;
  }
  if (dist < 1e-8) {
    stokes_self(v0, v1, v2, t, out);
  } else {
    for (int q = 0; q < d.nqf; ++q) {
      const V3 pt = {v0.x * d.qf[4 * q + 0] + v1.x * d.qf[4 * q + 1] + v2.x * d.qf[4 * q + 2],
                     v0.y * d.qf[4 * q + 0] + v1.y * d.qf[4 * q + 1] + v2.y * d.qf[4 * q + 2],
                     v0.z * d.qf[4 * q + 0] + v1.z * d.qf[4 * q + 1] + v2.z * d.qf[4 * q + 2]};
      stokeslet_point(out, d.qf[4 * q + 3] * A, t, pt);
    }
  }
  const double sc = 1. / 2 / d.mu;
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] *= sc;
}
__device__ inline void stokes_entry(const DevicePlan& d, V3 t, int tbc, int64_t j, double* out) {
  const int64_t N = d.n;
  const V3 c = {d.cx[j], d.cy[j], d.cz[j]};
  const V3 nrm = tbc ? V3{d.nx[j], d.ny[j], d.nz[j]} : V3{0, 0, 0};
  if (stokes_far_from(d, t, tbc, c, d.area[j], nrm,
                      [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; }, out))
    stokes_entry_near(d, t, tbc, j, out);
}

// The pressure of the single layer at a point t off the surface (include/fmmbem.h, "Field pressure"): three doubles per (target
// point, source panel j), the row vector pi with q += pi . f_j:
//   pi(t, s_j) = sum_q w_q A_j d_q / |d_q|^3,  d_q = t - y_q;   no mu, no 1/(2 mu)
// The regimes are those of a VELOCITY target above -- dist < 1e-8: pi = 0 (the mean of the one-sided limits +-2 pi n_j of a flat
// panel, its in-plane part neglected); sqrt(2 A) / dist >= 0.5: the K_fine rule on the vertices; else the K stored points -- and a
// point with |d_q|^2 < 1e-8 contributes 0, as in stokeslet_point.  One reciprocal square root per point, no division.
// In two parts like stokes_far_from / stokes_entry_near: stokes_pressure_far_from gives pi of a pair in the far regime (and the 0
// of a self pair) from a source panel held in registers or LDS, or says `deferred`; stokes_pressure_near the K_fine rule on the
// vertices of panel j.  The ONE text of pi: the near kernel of the pressure execute and fmmbem_kernel_pressure_entries
// (kernels_pressure.hip) both call it.
__device__ __forceinline__ void pressure_point(V3& out, double wA, V3 t, V3 pnt) {
  const V3 dd = sub(t, pnt);
  const double r2 = dd.x * dd.x + dd.y * dd.y + dd.z * dd.z;
  const double ri = rsqrt(r2);
  const double f = r2 < 1e-8 ? 0.0 : wA * (ri * ri * ri);
  out.x += f * dd.x; out.y += f * dd.y; out.z += f * dd.z;
}
template <class Quad>
__device__ __forceinline__ bool stokes_pressure_far_from(const DevicePlan& d, V3 t, V3 c, double A, Quad&& quad, V3& out) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  out = {0, 0, 0};
  // the regime by the expressions of stokes_far_from, dist < 1e-8 and sqrt(2 A) / dist >= 0.5; where 8 A < 0.99 dist^2 the exact
  // ratio is below 0.4975 and its roundings cannot lift it to 0.5 (see laplace_grad_from): no square root, no division there
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {
    const double dist = sqrt(d2);
    if (dist < 1e-8) return false;
    if (sqrt(2 * A) / dist >= 0.5) return true;
  }
  for (int q = 0; q < d.nq; ++q) pressure_point(out, d.qw[q] * A, t, quad(q));
  return false;
}
__device__ inline void stokes_pressure_near(const DevicePlan& d, V3 t, int64_t j, double A, V3& out) {
  const int64_t N = d.n;
  const V3 v0 = {d.vert[0 * N + j], d.vert[1 * N + j], d.vert[2 * N + j]};
  const V3 v1 = {d.vert[3 * N + j], d.vert[4 * N + j], d.vert[5 * N + j]};
  const V3 v2 = {d.vert[6 * N + j], d.vert[7 * N + j], d.vert[8 * N + j]};
  out = {0, 0, 0};
  for (int q = 0; q < d.nqf; ++q) {
    const V3 pt = {v0.x * d.qf[4 * q + 0] + v1.x * d.qf[4 * q + 1] + v2.x * d.qf[4 * q + 2],
                   v0.y * d.qf[4 * q + 0] + v1.y * d.qf[4 * q + 1] + v2.y * d.qf[4 * q + 2],
                   v0.z * d.qf[4 * q + 0] + v1.z * d.qf[4 * q + 1] + v2.z * d.qf[4 * q + 2]};
    pressure_point(out, d.qf[4 * q + 3] * A, t, pt);
  }
}
__device__ inline V3 stokes_pressure_entry(const DevicePlan& d, V3 t, int64_t j) {
  const int64_t N = d.n;
  const double A = d.area[j];
  V3 out;
  if (stokes_pressure_far_from(d, t, V3{d.cx[j], d.cy[j], d.cz[j]}, A,
                               [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; }, out))
    stokes_pressure_near(d, t, j, A, out);
  return out;
}

// The velocity gradient of the single layer at a point t off the surface (include/fmmbem.h, "Field velocity gradient"): per
// (target point, source panel j) with charge f the nine doubles G[3 k + m] = d u'_k / d t_m WITHOUT the 1/(2 mu),
//   G[k][m] += sum_q w_q A_j [ (-f_k d_m + delta_km s + d_k f_m) / r^3 - 3 s d_k d_m / r^5 ],   d = t - y_q,  s = d . f
// ADDED to G: the near kernel of the gradient execute contracts every point with the panel's f in place, straight into a row's
// nine sums; fmmbem_kernel_velocity_gradient_entries takes f = e_0, e_1, e_2 for the 27 numbers [k][m][e] (kernels_velgrad.hip).
// The regimes and the shortcut of the regime test are the pressure's above (dist < 1e-8: nothing added); a point with
// |d_q|^2 < 1e-8 adds 0.  One reciprocal square root per point, no division.  The ONE text of the tensor, in the two parts of
// the pressure: stokes_velgrad_far_from adds a pair in the far regime (nothing for a self pair) or says `deferred`;
// stokes_velgrad_near the K_fine rule on the vertices of panel j.
__device__ __forceinline__ void velgrad_point(double (&G)[9], double wA, V3 t, V3 pnt, V3 f) {
  const V3 dd = sub(t, pnt);
  const double r2 = dd.x * dd.x + dd.y * dd.y + dd.z * dd.z;
  const double ri = rsqrt(r2);
  const double ri2 = ri * ri;
  const double f3 = r2 < 1e-8 ? 0.0 : wA * (ri2 * ri);
  const double f5 = r2 < 1e-8 ? 0.0 : 3 * (wA * (ri2 * ri)) * ri2;
  const double s = dd.x * f.x + dd.y * f.y + dd.z * f.z;
  const double a = f3 * s, b = f5 * s;
  const double dv[3] = {dd.x, dd.y, dd.z}, fv[3] = {f.x, f.y, f.z};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int m = 0; m < 3; ++m)
      G[3 * k + m] += f3 * (dv[k] * fv[m] - fv[k] * dv[m]) + (k == m ? a : 0.0) - b * dv[k] * dv[m];
}
template <class Quad>
__device__ __forceinline__ bool stokes_velgrad_far_from(const DevicePlan& d, V3 t, V3 c, double A, Quad&& quad, V3 f, double (&G)[9]) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  // the regime by the expressions of stokes_pressure_far_from, with its shortcut: where 8 A < 0.99 dist^2 no square root, no division
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {
    const double dist = sqrt(d2);
    if (dist < 1e-8) return false;
    if (sqrt(2 * A) / dist >= 0.5) return true;
  }
  for (int q = 0; q < d.nq; ++q) velgrad_point(G, d.qw[q] * A, t, quad(q), f);
  return false;
}
__device__ inline void stokes_velgrad_near(const DevicePlan& d, V3 t, int64_t j, double A, V3 f, double (&G)[9]) {
  const int64_t N = d.n;
  const V3 v0 = {d.vert[0 * N + j], d.vert[1 * N + j], d.vert[2 * N + j]};
  const V3 v1 = {d.vert[3 * N + j], d.vert[4 * N + j], d.vert[5 * N + j]};
  const V3 v2 = {d.vert[6 * N + j], d.vert[7 * N + j], d.vert[8 * N + j]};
  for (int q = 0; q < d.nqf; ++q) {
    const V3 pt = {v0.x * d.qf[4 * q + 0] + v1.x * d.qf[4 * q + 1] + v2.x * d.qf[4 * q + 2],
                   v0.y * d.qf[4 * q + 0] + v1.y * d.qf[4 * q + 1] + v2.y * d.qf[4 * q + 2],
                   v0.z * d.qf[4 * q + 0] + v1.z * d.qf[4 * q + 1] + v2.z * d.qf[4 * q + 2]};
    velgrad_point(G, d.qf[4 * q + 3] * A, t, pt, f);
  }
}
// G = (1 / 2 mu) x the tensor of the pair (t, panel j) contracted with f: what fmmbem_kernel_velocity_gradient_entries returns
__device__ inline void stokes_velgrad_entry(const DevicePlan& d, V3 t, int64_t j, V3 f, double (&G)[9]) {
  const int64_t N = d.n;
  const double A = d.area[j];
  for (int c = 0; c < 9; ++c) G[c] = 0;
  if (stokes_velgrad_far_from(d, t, V3{d.cx[j], d.cy[j], d.cz[j]}, A,
                              [&](int q) { return V3{d.quad[(q * 3 + 0) * N + j], d.quad[(q * 3 + 1) * N + j], d.quad[(q * 3 + 2) * N + j]}; }, f, G))
    stokes_velgrad_near(d, t, j, A, f, G);
  const double sc = 1. / 2 / d.mu;
  for (int c = 0; c < 9; ++c) G[c] *= sc;
}

// The pressure and the velocity gradient of one pair TOGETHER (include/fmmbem.h, "Flow execute"): the regime test once -- the two
// quantities' tests are the same expressions -- and per point pressure_point's update of the pair's pi and velgrad_point's update of
// the nine sums, one after the other on the same t, point and weight.  Both are inlined here, so their common subexpressions --
// t - y_q, r2, the reciprocal square root, wA / r^3 -- are computed once; each keeps its own text above, and with it its bits.
// flow_far_from sets pi and adds to G for a pair in the far regime (pi = 0 and nothing added for a self pair) or says `deferred`;
// flow_near the K_fine rule on the vertices of panel j.
template <class Quad>
__device__ __forceinline__ bool stokes_flow_far_from(const DevicePlan& d, V3 t, V3 c, double A, Quad&& quad, V3 f, V3& pi, double (&G)[9]) {
  const V3 tc = sub(t, c);
  const double d2 = tc.x * tc.x + tc.y * tc.y + tc.z * tc.z;
  pi = {0, 0, 0};
  if (!(8 * A < 0.99 * d2 && d2 > 1e-15)) {
    const double dist = sqrt(d2);
    if (dist < 1e-8) return false;
    if (sqrt(2 * A) / dist >= 0.5) return true;
  }
  for (int q = 0; q < d.nq; ++q) {
    const double wA = d.qw[q] * A;
    const V3 pt = quad(q);
    pressure_point(pi, wA, t, pt);
    velgrad_point(G, wA, t, pt, f);
  }
  return false;
}
__device__ __forceinline__ void stokes_flow_near(const DevicePlan& d, V3 t, int64_t j, double A, V3 f, V3& pi, double (&G)[9]) {
  const int64_t N = d.n;
  const V3 v0 = {d.vert[0 * N + j], d.vert[1 * N + j], d.vert[2 * N + j]};
  const V3 v1 = {d.vert[3 * N + j], d.vert[4 * N + j], d.vert[5 * N + j]};
  const V3 v2 = {d.vert[6 * N + j], d.vert[7 * N + j], d.vert[8 * N + j]};
  pi = {0, 0, 0};
  for (int q = 0; q < d.nqf; ++q) {
    const V3 pt = {v0.x * d.qf[4 * q + 0] + v1.x * d.qf[4 * q + 1] + v2.x * d.qf[4 * q + 2],
                   v0.y * d.qf[4 * q + 0] + v1.y * d.qf[4 * q + 1] + v2.y * d.qf[4 * q + 2],
                   v0.z * d.qf[4 * q + 0] + v1.z * d.qf[4 * q + 1] + v2.z * d.qf[4 * q + 2]};
    const double wA = d.qf[4 * q + 3] * A;
    pressure_point(pi, wA, t, pt);
    velgrad_point(G, wA, t, pt, f);
  }
}

}  // namespace

}  // namespace fmmbem
