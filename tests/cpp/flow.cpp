// PlanAdapter::execute_flow and PlanAdapter::execute_stress on top of it (include/fmmbem/FMM_plan.hpp) on the owning plan that
// field_plan returns.
// usage: flow <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the points).  Charges: panel i carries (1 + (i % 7) / 4, (i % 5) / 8 - 0.25, 0.5 - (i % 3) / 4).
// Prints "single <status>" (a plan over its own panels must refuse), "traction <status>" (a field plan with a TRACTION point must
// refuse; its outputs stay as they were: "traction kept <0|1>"), "none <status>" (no output asked), then per order
//   "flow <n> <m> <p> <u> <q> <G>"        1 where the output of execute_flow with all three asked has the bits of execute(),
//                                         execute_pressure(), execute_velocity_gradient()
//   "subsets <p> <count of equal outputs> <count of outputs>"   over the six other combinations of null outputs
//   "stress <p> <0|1>"                    execute_stress against the composition of execute_pressure and execute_velocity_gradient
// and the velocity gradient of the last order, "gradient <n> <m> <p>" and nine doubles per line, for a comparison from outside.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

template <class T>
static int same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: flow <recursions> <points file>\n"); return 1; }
  int64_t m = 0;
  if (std::fread(&m, sizeof(m), 1, f) != 1 || m <= 0) return 1;
  std::vector<double> pts(3 * m);
  if (std::fread(pts.data(), sizeof(double), 3 * m, f) != (size_t)(3 * m)) return 1;
  std::fclose(f);
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  FMMOptions opts;
  opts.sparse_local = true;                             // as the drivers set it (examples/StokesBEM.cpp:147); a field plan needs it
  typedef StokesSphericalBEM::Panel Panel;
  typedef StokesSphericalBEM::point_type P;
  typedef StokesSphericalBEM::result_type U;
  typedef std::array<double, 9> T9;
  std::vector<Panel> panels;
  std::vector<P> points;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  for (int64_t i = 0; i < m; ++i) points.push_back(P{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]});
  std::vector<StokesSphericalBEM::charge_type> charges(n);
  for (size_t i = 0; i < n; ++i) charges[i] = StokesSphericalBEM::charge_type{1.0 + (double)(i % 7) / 4, (double)(i % 5) / 8 - 0.25, 0.5 - (double)(i % 3) / 4};
  StokesSphericalBEM K(8, 4, 1e-3);
  K.set_Kfine(19);
  try {
    FMM_plan<StokesSphericalBEM> single(K, panels, opts, 10);
    std::vector<U> u(2);
    std::vector<double> q(3, 7.0);
    std::vector<T9> g(1);
    int status = 0;
    try {
      single.execute_flow(charges, &u, &q, &g);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("single %d\n", status);
    std::vector<unsigned char> flags(points.size(), 0);
    flags[1] = 1;
    status = 0;
    try {
      single.field_plan(points, flags)->execute_flow(charges, nullptr, &q, nullptr);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("traction %d\n", status);
    std::printf("traction kept %d\n", (int)(u.size() == 2 && q.size() == 3 && q[0] == 7.0 && q[2] == 7.0 && g.size() == 1));
    auto field = single.field_plan(points);
    status = 0;
    try {
      field->execute_flow(charges, nullptr, nullptr, nullptr);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("none %d\n", status);
    std::vector<T9> last;
    for (int p : {8, 10}) {
      field->kernel().set_p(p);
      const std::vector<U> u1 = field->execute(charges);
      const std::vector<double> q1 = field->execute_pressure(charges);
      const std::vector<T9> g1 = field->execute_velocity_gradient(charges);
      field->execute_flow(charges, &u, &q, &g);
      std::printf("flow %zu %zu %d %d %d %d\n", n, g.size(), p, same(u, u1), same(q, q1), same(g, g1));
      int equal = 0, count = 0;
      for (int mask = 1; mask < 7; ++mask) {
        std::vector<U> u2;
        std::vector<double> q2;
        std::vector<T9> g2;
        field->execute_flow(charges, mask & 1 ? &u2 : nullptr, mask & 2 ? &q2 : nullptr, mask & 4 ? &g2 : nullptr);
        if (mask & 1) { ++count; equal += same(u2, u1); } else equal -= !u2.empty();
        if (mask & 2) { ++count; equal += same(q2, q1); } else equal -= !q2.empty();
        if (mask & 4) { ++count; equal += same(g2, g1); } else equal -= !g2.empty();
      }
      std::printf("subsets %d %d %d\n", p, equal, count);
      std::vector<T9> s1 = g1;                          // the stress as two single executes composed it
      for (size_t i = 0; i < s1.size(); ++i)
        for (int k = 0; k < 3; ++k)
          for (int c = 0; c < 3; ++c) s1[i][3 * k + c] = -q1[i] * (k == c ? 1.0 : 0.0) + K.Mu * (g1[i][3 * k + c] + g1[i][3 * c + k]);
      std::printf("stress %d %d\n", p, same(field->execute_stress(charges), s1));
      last = g;
      if (p == 10) {
        std::printf("gradient %zu %zu %d\n", n, last.size(), p);
        for (const auto& row : last)
          for (int c = 0; c < 9; ++c) std::printf(c == 8 ? "%.17g\n" : "%.17g ", row[c]);
      }
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
