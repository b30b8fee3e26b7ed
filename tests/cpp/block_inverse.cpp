// fmmbem::BlockInversePC (fmmbem_plan_block_inverse_* through the adapter).  usage: block_inverse <recursions>
// First-kind Laplace plan on a unit sphere at p = 10; v(i) = 1 / |c_i - q| at the panel centroids c_i for a charge q inside.
// Prints "block_inverse <n> <bytes of the inverses>", then the blocks
//   "v"      the vector, "z" = M(v, z) of the functor,
//   "gmres"  iterations, residual, the orders and the solution of fmmbem::GMRES(plan, x, v, options, M),
// every number as %.17g; the driver (tests/test_cpp_block_inverse.py) holds them against the Python calls on the same mesh.
// Without a device: "error <status> ..." and 2.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

struct SolverOptions {            // the members of examples/BEM/SolverOptions.hpp the adapter reads
  double residual = 1e-6;
  int max_iters = 60, restart = 60;
  unsigned max_p = 10;
  bool variable_p = true;
};

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  const double q[3] = {0.3, 0.2, 0.1};
  std::vector<double> b(n);
  for (size_t i = 0; i < n; ++i) {
    double d2 = 0;
    for (int c = 0; c < 3; ++c) {
      const double cc = (v[9 * i + c] + v[9 * i + 3 + c] + v[9 * i + 6 + c]) / 3 - q[c];
      d2 += cc * cc;
    }
    b[i] = 1.0 / std::sqrt(d2);
  }
  FMMOptions opts;
  opts.sparse_local = true;
  LaplaceSphericalBEM K(10, 3);
  SolverOptions so;
  fmmbem::solver_output() = false;
  try {
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, opts);
    fmmbem::BlockInversePC<LaplaceSphericalBEM> M(K, panels, opts);
    std::printf("block_inverse %zu %lld\n", n, (long long)M.bytes());
    std::vector<double> z;
    M(b, z);
    std::printf("v\n");
    for (double t : b) std::printf("%.17g\n", t);
    std::printf("z\n");
    for (double t : z) std::printf("%.17g\n", t);
    std::vector<double> x(n, 0.0);
    const fmmbem::SolveReport rep = fmmbem::GMRES(plan, x, b, so, M);
    std::printf("gmres\niterations %d residual %.17g\n", rep.iterations, rep.residual);
    for (size_t i = 0; i < rep.p.size(); ++i) std::printf("p %d %.17g\n", rep.p[i], rep.resid[i]);
    for (double t : x) std::printf("%.17g\n", t);
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
