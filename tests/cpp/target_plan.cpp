// The reference's four-argument constructor FMM_plan(K, sources, targets, opts) (include/FMM_plan.hpp:45-55) through the adapter:
// the exterior point of examples/LaplaceBEM.cpp:346-369 generalised to many targets.  usage: target_plan <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the target points), then m doubles (their flags, 0 or 1).  Charges: 1 + (i % 7) / 4.
// Prints "stokes <status>" (the Stokes constructor must refuse), then "targets <n> <m> <p>" and one result per line per order.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: target_plan <recursions> <targets file>\n"); return 1; }
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
  // Stokes: refused before anything touches a device
  {
    typedef StokesSphericalBEM::Panel SPanel;
    typedef StokesSphericalBEM::point_type SP;
    std::vector<SPanel> sp, st;
    for (size_t i = 0; i < n; ++i)
      sp.emplace_back(SP{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, SP{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, SP{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
    st.emplace_back(SP{3., 3., 3.}, SP{3., 3., 3.}, SP{3., 3., 3.});
    StokesSphericalBEM KS(5, 3, 1e-3);
    int status = 0;
    try {
      FMM_plan<StokesSphericalBEM> splan(KS, sp, st, opts);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("stokes %d\n", status);
  }
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels, targets;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  for (int64_t i = 0; i < m; ++i) {
    const P t{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    targets.emplace_back(t, t, t);                      // as the driver makes its exterior point (LaplaceBEM.cpp:348-349) ...
    targets.back().center = t;                          // ... with the centre set exactly (:350)
    if (flags[i] != 0) targets.back().switch_BC();
  }
  std::vector<double> charges(n);
  for (size_t i = 0; i < n; ++i) charges[i] = 1.0 + (double)(i % 7) / 4;
  LaplaceSphericalBEM K(10, 3);
  try {
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, targets, opts, 12);
    for (int p : {10, 12}) {
      plan.kernel().set_p(p);
      std::vector<double> res = plan.execute(charges);
      std::printf("targets %zu %zu %d\n", n, res.size(), p);
      for (double x : res) std::printf("%.17g\n", x);
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
