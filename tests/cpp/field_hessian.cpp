// PlanAdapter::execute_hessian (include/fmmbem/FMM_plan.hpp) on a plan over separate targets and on a field plan.
// usage: field_hessian <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the target points), then m doubles (their flags, 0 or 1).  Charges: 1 + (i % 7) / 4.
// Prints "single <status>" (a plan over its own panels must refuse), then "targets <n> <m> <p>" and one Hessian, nine numbers
// row-major, per line per order, then "field <n> <m> <p>" and the same rows from the field plan.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

static void print_rows(const std::vector<std::array<double, 9>>& h) {
  for (const auto& x : h) {
    for (int c = 0; c < 9; ++c) std::printf(c ? " %.17g" : "%.17g", x[c]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: field_hessian <recursions> <targets file>\n"); return 1; }
  int64_t m = 0;
  if (std::fread(&m, sizeof(m), 1, f) != 1 || m <= 0) return 1;
  std::vector<double> pts(3 * m), flags(m);
  if (std::fread(pts.data(), sizeof(double), 3 * m, f) != (size_t)(3 * m) || std::fread(flags.data(), sizeof(double), m, f) != (size_t)m) return 1;
  std::fclose(f);
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  FMMOptions opts;
  opts.sparse_local = true;                             // as the drivers set it (examples/LaplaceBEM.cpp:81); a field plan needs it
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels, targets;
  std::vector<P> points;
  std::vector<unsigned char> point_flags;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  for (int64_t i = 0; i < m; ++i) {
    const P t{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    targets.emplace_back(t, t, t);
    targets.back().center = t;
    if (flags[i] != 0) targets.back().switch_BC();
    points.push_back(t);
    point_flags.push_back(flags[i] != 0);
  }
  std::vector<double> charges(n);
  for (size_t i = 0; i < n; ++i) charges[i] = 1.0 + (double)(i % 7) / 4;
  LaplaceSphericalBEM K(10, 3);
  try {
    FMM_plan<LaplaceSphericalBEM> single(K, panels, opts, 12);
    int status = 0;
    try {
      single.execute_hessian(charges);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("single %d\n", status);
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, targets, opts, 12);
    for (int p : {10, 12}) {
      plan.kernel().set_p(p);
      const std::vector<std::array<double, 9>> h = plan.execute_hessian(charges);
      std::printf("targets %zu %zu %d\n", n, h.size(), p);
      print_rows(h);
    }
    auto field = single.field_plan(points, point_flags);
    field->kernel().set_p(12);
    const std::vector<std::array<double, 9>> h = field->execute_hessian(charges);
    std::printf("field %zu %zu %d\n", n, h.size(), 12);
    print_rows(h);
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
