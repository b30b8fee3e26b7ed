// FMMOptions::near_f32_max_p through the adapter (fmmbem_options.near_f32_max_p).  usage: near_f32 <recursions> <threshold>
// Laplace plan on a unit sphere (sparse_local, as examples/LaplaceBEM.cpp:81), charges x[i] = 1 + (i % 7) / 4, one execute per order
// p = 1 .. 8.  Prints "near_f32 <n> <threshold> <near_f32_bytes>", then per order "p <p> last_near_f32 <0|1> sum <sum of the
// result>".  Without a device: "error <status> ..." and 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  const int threshold = argc > 2 ? std::atoi(argv[2]) : 4;
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  std::vector<double> charges(n);
  for (size_t i = 0; i < n; ++i) charges[i] = 1.0 + (double)(i % 7) / 4;
  FMMOptions opts;
  opts.sparse_local = true;
  opts.set_near_f32_max_p(threshold);
  LaplaceSphericalBEM K(8, 3);
  try {
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, opts);
    fmmbem_stats st;
    fmmbem::check(fmmbem_plan_stats(plan.handle(), &st));
    std::printf("near_f32 %zu %d %lld\n", n, threshold, (long long)st.near_f32_bytes);
    for (int p = 1; p <= 8; ++p) {
      plan.kernel().set_p(p);
      const std::vector<double> y = plan.execute(charges);
      fmmbem::check(fmmbem_plan_stats(plan.handle(), &st));
      double sum = 0;
      for (double x : y) sum += x;
      std::printf("p %d last_near_f32 %d sum %.17g\n", p, (int)st.last_near_f32, sum);
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
