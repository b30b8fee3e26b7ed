// fmmbem::DirectSum's field quantities (include/fmmbem/Direct.hpp): gradient on a Laplace kernel, pressure, velocity_gradient and
// stress on a Stokes kernel, and the cross-kernel calls, which throw the library's refusal.
// usage: direct_field <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the target points), then m doubles (their flags, 0 or 1).
// Charges: Laplace 1 + (i % 7) / 4; Stokes (1 + (i % 7) / 4, -0.5 + (i % 3), 0.25 (i % 5)).  Prints, one value per line:
//   "gradient <n> <m>"            DirectSum<LaplaceSphericalBEM>::gradient(charges, targets), 3 values per target
//   "laplace_refuses"             the status of the Error thrown by pressure, velocity_gradient and stress on the Laplace kernel
//   "pressure <n> <m>"            DirectSum<StokesSphericalBEM>::pressure(charges, targets)
//   "velocity_gradient <m>"       ...::velocity_gradient, 9 values per target
//   "stress <m>"                  ...::stress, 9 values per target
//   "stokes_refuses"              the status of the Error thrown by gradient on the Stokes kernel
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/Direct.hpp"

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

template <class F>
static void refused(F&& call) {
  try {
    call();
    std::printf("0\n");
  } catch (const fmmbem::Error& e) {
    std::printf("%d\n", e.status);
  }
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: direct_field <recursions> <targets file>\n"); return 1; }
  int64_t m = 0;
  if (std::fread(&m, sizeof(m), 1, f) != 1 || m < 1) return 1;
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
      const auto g = D.gradient(charges, targets);
      std::printf("gradient %zu %zu\n", n, g.size());
      for (const auto& x : g) std::printf("%.17g\n%.17g\n%.17g\n", x[0], x[1], x[2]);
      std::printf("laplace_refuses\n");
      refused([&] { D.pressure(charges, targets); });
      refused([&] { D.velocity_gradient(charges, targets); });
      refused([&] { D.stress(charges, targets); });
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
      const std::vector<double> q = D.pressure(charges, targets);
      std::printf("pressure %zu %zu\n", n, q.size());
      for (double x : q) std::printf("%.17g\n", x);
      const auto g = D.velocity_gradient(charges, targets);
      std::printf("velocity_gradient %zu\n", g.size());
      for (const auto& a : g) for (double x : a) std::printf("%.17g\n", x);
      const auto s = D.stress(charges, targets);
      std::printf("stress %zu\n", s.size());
      for (const auto& a : s) for (double x : a) std::printf("%.17g\n", x);
      std::printf("stokes_refuses\n");
      refused([&] { D.gradient(charges, targets); });
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
