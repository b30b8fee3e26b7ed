// PlanAdapter::execute_velocity_gradient and PlanAdapter::execute_stress (include/fmmbem/FMM_plan.hpp) on the owning plan that
// field_plan returns.
// usage: field_velocity_gradient <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the points).  Charges: panel i carries (1 + (i % 7) / 4, (i % 5) / 8 - 0.25, 0.5 - (i % 3) / 4).
// Prints "single <status>" (a plan over its own panels must refuse), "traction <status>" (a field plan with a TRACTION point must
// refuse), then per order "gradient <n> <m> <p>" and nine doubles per line, "stress <n> <m> <p>" and nine doubles per line.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

static void print_rows(const std::vector<std::array<double, 9>>& rows) {
  for (const auto& g : rows) {
    for (int c = 0; c < 9; ++c) std::printf(c == 8 ? "%.17g\n" : "%.17g ", g[c]);
  }
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: field_velocity_gradient <recursions> <points file>\n"); return 1; }
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
    int status = 0;
    try {
      single.execute_velocity_gradient(charges);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("single %d\n", status);
    std::vector<unsigned char> flags(points.size(), 0);
    flags[1] = 1;
    status = 0;
    try {
      single.field_plan(points, flags)->execute_stress(charges);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("traction %d\n", status);
    auto field = single.field_plan(points);
    for (int p : {8, 10}) {
      field->kernel().set_p(p);
      const auto g = field->execute_velocity_gradient(charges);
      std::printf("gradient %zu %zu %d\n", n, g.size(), p);
      print_rows(g);
      const auto s = field->execute_stress(charges);
      std::printf("stress %zu %zu %d\n", n, s.size(), p);
      print_rows(s);
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
