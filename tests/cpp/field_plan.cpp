// PlanAdapter::field_plan through the header-only adapter: the field of a layer at points of their own, Laplace and Stokes.
// usage: field_plan <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the points), then m doubles (their flags, 0 or 1).
// Charges: Laplace 1 + (i % 7) / 4; Stokes (1 + (i % 7) / 4, -0.5 + (i % 5) / 8, 0.25 (i % 3)).
// Prints "four-argument stokes <status>" (that constructor must keep refusing), "field of field <status>" (a field plan has no field
// plan), then per kernel and order "laplace <n> <m> <p>" / "stokes <n> <m> <p>" and one result (Stokes: three numbers) per line; the
// last order of each kernel is above the operator plan's p_max (the field plan grows), and is followed by "batch <k>" with the
// results of execute_batch on two vectors (the charges and their negatives).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

template <class Kernel>
static std::vector<typename Kernel::Panel> panels_of(const std::vector<double>& v) {
  typedef typename Kernel::point_type P;
  std::vector<typename Kernel::Panel> out;
  for (size_t i = 0; i < v.size() / 9; ++i)
    out.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  return out;
}

static void print(const std::vector<double>& r) { for (double x : r) std::printf("%.17g\n", x); }
static void print(const std::vector<Vec<3, double>>& r) { for (const auto& x : r) std::printf("%.17g %.17g %.17g\n", x[0], x[1], x[2]); }

template <class Kernel, class Charges>
static void run(const char* name, Kernel K, const std::vector<double>& v, const std::vector<double>& pts, const std::vector<double>& flags,
                const Charges& charges, int p_grown) {
  typedef typename Kernel::point_type P;
  FMMOptions opts;
  opts.sparse_local = true;
  const size_t m = flags.size();
  std::vector<P> points;
  std::vector<unsigned char> fl;
  for (size_t i = 0; i < m; ++i) { points.push_back(P{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}); fl.push_back(flags[i] != 0); }
  FMM_plan<Kernel> plan(K, panels_of<Kernel>(v), opts);
  auto field = plan.field_plan(points, fl);
  int status = 0;
  try { field->field_plan(points, fl); } catch (const fmmbem::Error& e) { status = e.status; }
  std::printf("field of field %d\n", status);
  for (int p : {K.p(), p_grown}) {
    field->kernel().set_p(p);                              // p_grown > p_max: the field plan grows, as every plan does
    auto res = field->execute(charges);
    std::printf("%s %zu %zu %d\n", name, charges.size(), res.size(), p);
    print(res);
  }
  Charges neg = charges;
  for (auto& c : neg) c = c * -1.0;
  auto both = field->execute_batch({charges, neg});
  std::printf("batch %zu\n", both.size());
  for (const auto& r : both) print(r);
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: field_plan <recursions> <points file>\n"); return 1; }
  int64_t m = 0;
  if (std::fread(&m, sizeof(m), 1, f) != 1 || m <= 0) return 1;
  std::vector<double> pts(3 * m), flags(m);
  if (std::fread(pts.data(), sizeof(double), 3 * m, f) != (size_t)(3 * m) || std::fread(flags.data(), sizeof(double), m, f) != (size_t)m) return 1;
  std::fclose(f);
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  {
    // the reference-shaped four-argument constructor keeps refusing Stokes, before anything touches a device
    typedef StokesSphericalBEM::Panel SPanel;
    typedef StokesSphericalBEM::point_type SP;
    std::vector<SPanel> st;
    st.emplace_back(SP{3., 3., 3.}, SP{3., 3., 3.}, SP{3., 3., 3.});
    FMMOptions opts;
    StokesSphericalBEM KS(5, 3, 1e-3);
    int status = 0;
    try {
      FMM_plan<StokesSphericalBEM> splan(KS, panels_of<StokesSphericalBEM>(v), st, opts);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("four-argument stokes %d\n", status);
  }
  try {
    std::vector<double> q(n);
    for (size_t i = 0; i < n; ++i) q[i] = 1.0 + (double)(i % 7) / 4;
    run("laplace", LaplaceSphericalBEM(8, 3), v, pts, flags, q, 11);
    std::vector<Vec<3, double>> g(n);
    for (size_t i = 0; i < n; ++i) g[i] = Vec<3, double>(1.0 + (double)(i % 7) / 4, -0.5 + (double)(i % 5) / 8, 0.25 * (double)(i % 3));
    StokesSphericalBEM KS(6, 4, 1e-3);
    KS.K_fine = 19;
    run("stokes", KS, v, pts, flags, g, 9);
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
