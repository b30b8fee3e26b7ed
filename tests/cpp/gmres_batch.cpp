// fmmbem::GMRES_batch / FGMRES_batch (fmmbem_gmres_batch through the adapter).  usage: gmres_batch <recursions> <k> <mode>
// mode: gmres | fgmres | gmres_diag | fgmres_diag (the last two with a diagonal functor the adapter has to probe).
// First-kind Laplace plan on a unit sphere; b_j(i) = 1 / |c_i - q_j| at the panel centroids c_i for charges q_j inside the sphere,
// q_0 at the centre (b nearly constant: few iterations), the others further and further out (more iterations).
// Prints "systems <n> <k> <mode>", then for every system a block "single <j>" from fmmbem::GMRES on it alone and, after all of
// them, a block "batch <j>" from the batched call: iterations, residual, the orders, the solution, every number as %.17g.  The
// driver (tests/test_cpp_gmres_batch.py) compares the blocks as text.  Without a device: "error <status> ..." and 2.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

struct SolverOptions {            // the members of examples/BEM/SolverOptions.hpp the adapter reads
  double residual = 1e-6;
  int max_iters = 60, restart = 60;
  unsigned max_p = 10;
  bool variable_p = true;
};

struct Scale {                    // Preconditioners::Diagonal's shape: y = r .* x
  std::vector<double> r;
  void operator()(const std::vector<double>& x, std::vector<double>& y) const {
    y.resize(x.size());
    for (size_t i = 0; i < x.size(); ++i) y[i] = r[i] * x[i];
  }
};

static void print_block(const char* tag, int j, const fmmbem::SolveReport& rep, const std::vector<double>& x) {
  std::printf("%s %d\n", tag, j);
  std::printf("iterations %d residual %.17g\n", rep.iterations, rep.residual);
  for (size_t i = 0; i < rep.p.size(); ++i) std::printf("p %d %.17g\n", rep.p[i], rep.resid[i]);
  for (double v : x) std::printf("%.17g\n", v);
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  const int k = argc > 2 ? std::atoi(argv[2]) : 3;
  const std::string mode = argc > 3 ? argv[3] : "gmres";
  const bool flexible = mode.rfind("fgmres", 0) == 0, diag = mode.find("_diag") != std::string::npos;
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  std::vector<std::vector<double>> B(k, std::vector<double>(n));
  for (int j = 0; j < k; ++j) {
    const double q[3] = {k > 1 ? 0.9 * j / (k - 1) : 0.0, 0.0, 0.0};
    for (size_t i = 0; i < n; ++i) {
      double d2 = 0;
      for (int c = 0; c < 3; ++c) {
        const double cc = (v[9 * i + c] + v[9 * i + 3 + c] + v[9 * i + 6 + c]) / 3 - q[c];
        d2 += cc * cc;
      }
      B[j][i] = 1.0 / std::sqrt(d2);
    }
  }
  FMMOptions opts;
  opts.sparse_local = true;
  LaplaceSphericalBEM K(10, 3);
  SolverOptions so;
  fmmbem::solver_output() = false;
  try {
    FMM_plan<LaplaceSphericalBEM> plan(K, panels, opts);
    Scale M;
    if (diag) {
      M.r.resize(n);
      fmmbem::check(fmmbem_plan_get_diagonal(plan.handle(), M.r.data()));
      for (double& d : M.r) d = 1.0 / d;
    }
    std::printf("systems %zu %d %s\n", n, k, mode.c_str());
    for (int j = 0; j < k; ++j) {
      std::vector<double> x(n, 0.0);
      plan.kernel().set_p(10);                          // every solve starts from the construction order, as the batch does
      fmmbem::SolveReport rep;
      if (flexible) rep = diag ? fmmbem::FGMRES(plan, x, B[j], so, M) : fmmbem::FGMRES(plan, x, B[j], so);
      else rep = diag ? fmmbem::GMRES(plan, x, B[j], so, M) : fmmbem::GMRES(plan, x, B[j], so);
      print_block("single", j, rep, x);
    }
    plan.kernel().set_p(10);
    std::vector<std::vector<double>> X(k, std::vector<double>(n, 0.0));
    std::vector<fmmbem::SolveReport> reps;
    if (flexible) reps = diag ? fmmbem::FGMRES_batch(plan, X, B, so, M) : fmmbem::FGMRES_batch(plan, X, B, so);
    else reps = diag ? fmmbem::GMRES_batch(plan, X, B, so, M) : fmmbem::GMRES_batch(plan, X, B, so);
    for (int j = 0; j < k; ++j) print_block("batch", j, reps[j], X[j]);
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
