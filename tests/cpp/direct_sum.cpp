// fmmbem::DirectSum / fmmbem::direct_matvec (include/fmmbem/Direct.hpp) beside the reference-named Direct::matvec of the compat header.
// usage: direct_sum <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the target points), then m doubles (their flags, 0 or 1).
// Charges: Laplace 1 + (i % 7) / 4; Stokes (1 + (i % 7) / 4, -0.5 + (i % 3), 0.25 (i % 5)).  Prints, one value per line:
//   "laplace <n> <m>"      DirectSum<LaplaceSphericalBEM>::matvec(charges, targets)
//   "laplace_add <m>"      direct_matvec into results preset to 1.5
//   "laplace_compat 16"    Direct::matvec (compat header) at the first 16 targets
//   "laplace_sym <n>"      the symmetric form, every third panel NORMAL_DERIV
//   "stokes <n> <m>"       DirectSum<StokesSphericalBEM>::matvec(charges, targets), 3 values per target
//   "stokes_add <m>"       direct_matvec into results preset to (1.5, 1.5, 1.5)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/Direct.hpp"
#include "fmmbem/compat/Direct.hpp"

template <class Kernel>
static void make(const std::vector<double>& v, const std::vector<double>& pts, const std::vector<double>& flags,
                 std::vector<typename Kernel::source_type>& panels, std::vector<typename Kernel::target_type>& targets) {
  typedef typename Kernel::point_type P;
  for (size_t i = 0; i < v.size() / 9; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  for (size_t i = 0; i < flags.size(); ++i) {
    const P t{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    targets.emplace_back(t, t, t);
    targets.back().center = t;
    if (flags[i] != 0) targets.back().switch_BC();
  }
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: direct_sum <recursions> <targets file>\n"); return 1; }
  int64_t m = 0;
  if (std::fread(&m, sizeof(m), 1, f) != 1 || m < 16) return 1;
  std::vector<double> pts(3 * m), flags(m);
  if (std::fread(pts.data(), sizeof(double), 3 * m, f) != (size_t)(3 * m) || std::fread(flags.data(), sizeof(double), m, f) != (size_t)m) return 1;
  std::fclose(f);
  size_t n = 0;
  fmmbem::check(fmmbem_mesh_unit_sphere(r, nullptr, &n));
  std::vector<double> v(9 * n);
  fmmbem::check(fmmbem_mesh_unit_sphere(r, v.data(), &n));
  try {
    {
      LaplaceSphericalBEM K(5, 3);
      std::vector<LaplaceSphericalBEM::Panel> panels, targets;
      make<LaplaceSphericalBEM>(v, pts, flags, panels, targets);
      std::vector<double> charges(n);
      for (size_t i = 0; i < n; ++i) charges[i] = 1.0 + (double)(i % 7) / 4;
      fmmbem::DirectSum<LaplaceSphericalBEM> D(K, panels);
      const std::vector<double> y = D.matvec(charges, targets);
      std::printf("laplace %zu %zu\n", n, y.size());
      for (double x : y) std::printf("%.17g\n", x);
      std::vector<double> acc(targets.size(), 1.5);
      fmmbem::direct_matvec(K, panels, charges, targets, acc);
      std::printf("laplace_add %zu\n", acc.size());
      for (double x : acc) std::printf("%.17g\n", x);
      const std::vector<LaplaceSphericalBEM::Panel> few(targets.begin(), targets.begin() + 16);
      std::vector<double> old(16, 0.0);
      Direct::matvec(K, panels, charges, few, old);
      std::printf("laplace_compat 16\n");
      for (double x : old) std::printf("%.17g\n", x);
      for (size_t i = 0; i < n; i += 3) panels[i].switch_BC();
      fmmbem::DirectSum<LaplaceSphericalBEM> S(K, panels);
      const std::vector<double> ys = S.matvec(charges);
      std::printf("laplace_sym %zu\n", ys.size());
      for (double x : ys) std::printf("%.17g\n", x);
    }
    {
      StokesSphericalBEM K(5, 4, 1e-3);
      K.set_Kfine(19);
      std::vector<StokesSphericalBEM::Panel> panels, targets;
      make<StokesSphericalBEM>(v, pts, flags, panels, targets);
      typedef StokesSphericalBEM::charge_type C3;
      std::vector<C3> charges(n);
      for (size_t i = 0; i < n; ++i) charges[i] = C3(1.0 + (double)(i % 7) / 4, -0.5 + (double)(i % 3), 0.25 * (double)(i % 5));
      fmmbem::DirectSum<StokesSphericalBEM> D(K, panels);
      const std::vector<StokesSphericalBEM::result_type> y = D.matvec(charges, targets);
      std::printf("stokes %zu %zu\n", n, y.size());
      for (const auto& x : y) std::printf("%.17g\n%.17g\n%.17g\n", x[0], x[1], x[2]);
      std::vector<StokesSphericalBEM::result_type> acc(targets.size(), StokesSphericalBEM::result_type(1.5, 1.5, 1.5));
      fmmbem::direct_matvec(K, panels, charges, targets, acc);
      std::printf("stokes_add %zu\n", acc.size());
      for (const auto& x : acc) std::printf("%.17g\n%.17g\n%.17g\n", x[0], x[1], x[2]);
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
