// PlanAdapter::execute_batch (fmmbem_plan_execute_batch through the adapter).  usage: batch <recursions> <k> <p>
// Laplace plan on a unit sphere (sparse_local, as examples/LaplaceBEM.cpp:81), k charge vectors x_j[i] = 1 + ((i + 3 j) % 7) / 4.
// Prints "mismatch <status>" (a wrong-length vector must throw), "batch <n> <k> <p>", "equal <0|1>" (every batch result bit for
// bit the single execute of its vector), then the k results, one value per line.  Without a device: "error <status> ..." and 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  const int k = argc > 2 ? std::atoi(argv[2]) : 3;
  const int p = argc > 3 ? std::atoi(argv[3]) : 8;
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  std::vector<std::vector<double>> charges(k, std::vector<double>(n));
  for (int j = 0; j < k; ++j)
    for (size_t i = 0; i < n; ++i) charges[j][i] = 1.0 + (double)((i + 3 * j) % 7) / 4;
  FMMOptions opts;
  opts.sparse_local = true;
  LaplaceSphericalBEM K(5, 3);
  try {
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, opts);
    {
      std::vector<std::vector<double>> bad = charges;
      bad.back().pop_back();
      int status = 0;
      try {
        plan.execute_batch(bad);
      } catch (const fmmbem::Error& e) {
        status = e.status;
      }
      std::printf("mismatch %d\n", status);
    }
    plan.kernel().set_p(p);                             // above the plan's size (5): execute_batch grows it as execute does
    const std::vector<std::vector<double>> res = plan.execute_batch(charges);
    bool equal = res.size() == (size_t)k;
    for (int j = 0; j < k && equal; ++j) {
      const std::vector<double> one = plan.execute(charges[j]);
      equal = one.size() == res[j].size() && std::memcmp(one.data(), res[j].data(), one.size() * sizeof(double)) == 0;
    }
    std::printf("batch %zu %d %d\n", n, k, p);
    std::printf("equal %d\n", equal ? 1 : 0);
    for (const auto& y : res)
      for (double x : y) std::printf("%.17g\n", x);
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
