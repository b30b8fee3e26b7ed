// PlanAdapter::execute_representation (include/fmmbem/FMM_plan.hpp) on the owning plan that field_plan returns.
// usage: representation <recursions> <file>
// <file>: int64 m, then m x 3 doubles (the points).  Density: panel i carries 1 + (i % 7) / 4; surface potential: (i % 5) / 8 - 0.25.
// Prints "single <status>" (a plan over its own panels must refuse; its outputs stay as they were: "single kept <0|1>"),
// "no layer <status>" and "no output <status>", then per order
//   "representation <n> <m> <p> <phi error> <grad error>"   the largest |result - (S - D)| over the points, relative to the larger of
//                                      the two layers' largest entries: S, D the adapter's execute() on an all-POTENTIAL and an
//                                      all-NORMAL_DERIV field plan over the points, and the same with execute_gradient()
//   "subsets <p> <count of equal outputs> <count of outputs>"   missing outputs leave the other's bits; a missing layer is a zero
//                                      vector (to 1e-12 of the scale)
// and the gradient of the last order, "gradient <n> <m> <p>" and three doubles per line, for a comparison from outside.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

typedef Vec<3, double> V3;

template <class T>
static int same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

// the largest |got - (s - d)| relative to the larger of max |s|, max |d|
static double error_of(const std::vector<double>& got, const std::vector<double>& s, const std::vector<double>& d) {
  if (got.size() != s.size() || got.size() != d.size() || got.empty()) return 1e300;
  double err = 0, top = 0;
  for (size_t i = 0; i < got.size(); ++i) {
    err = std::max(err, std::fabs(got[i] - (s[i] - d[i])));
    top = std::max(top, std::max(std::fabs(s[i]), std::fabs(d[i])));
  }
  return err / top;
}
static std::vector<double> flat(const std::vector<V3>& g) {
  std::vector<double> out;
  for (const auto& x : g) for (int c = 0; c < 3; ++c) out.push_back(x[c]);
  return out;
}

int main(int argc, char** argv) {
  const int r = argc > 1 ? std::atoi(argv[1]) : 4;
  FILE* f = argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  if (!f) { std::printf("usage: representation <recursions> <points file>\n"); return 1; }
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
  opts.sparse_local = true;                             // as the drivers set it (examples/LaplaceBEM.cpp:81); a field plan needs it
  typedef LaplaceSphericalBEM::Panel Panel;
  typedef LaplaceSphericalBEM::point_type P;
  std::vector<Panel> panels;
  std::vector<P> points;
  for (size_t i = 0; i < n; ++i)
    panels.emplace_back(P{v[9 * i], v[9 * i + 1], v[9 * i + 2]}, P{v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]}, P{v[9 * i + 6], v[9 * i + 7], v[9 * i + 8]});
  for (int64_t i = 0; i < m; ++i) points.push_back(P{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]});
  std::vector<double> sigma(n), mu(n);
  for (size_t i = 0; i < n; ++i) { sigma[i] = 1.0 + (double)(i % 7) / 4; mu[i] = (double)(i % 5) / 8 - 0.25; }
  const std::vector<double> none(n, 0.0);
  LaplaceSphericalBEM K(10, 3);
  try {
    FMM_plan<LaplaceSphericalBEM> single(K, panels, opts, 12);
    std::vector<double> phi(3, 7.0);
    std::vector<V3> grad(2);
    int status = 0;
    try {
      single.execute_representation(&sigma, &mu, &phi, &grad);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("single %d\n", status);
    std::printf("single kept %d\n", (int)(phi.size() == 3 && phi[0] == 7.0 && phi[2] == 7.0 && grad.size() == 2));
    std::vector<unsigned char> mixed(points.size(), 0), all0(points.size(), 0), all1(points.size(), 1);
    for (size_t i = 0; i < mixed.size(); i += 3) mixed[i] = 1;
    auto field = single.field_plan(points, mixed);        // the representation execute: the points' flags do not enter
    auto layer0 = single.field_plan(points, all0), layer1 = single.field_plan(points, all1);
    status = 0;
    try {
      field->execute_representation(nullptr, nullptr, &phi, &grad);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("no layer %d\n", status);
    status = 0;
    try {
      field->execute_representation(&sigma, &mu, nullptr, nullptr);
    } catch (const fmmbem::Error& e) {
      status = e.status;
    }
    std::printf("no output %d\n", status);
    for (int p : {8, 12}) {
      for (auto* pl : {field.get(), layer0.get(), layer1.get()}) pl->kernel().set_p(p);
      const std::vector<double> S = layer0->execute(sigma), D = layer1->execute(mu);
      const std::vector<double> gS = flat(layer0->execute_gradient(sigma)), gD = flat(layer1->execute_gradient(mu));
      field->execute_representation(&sigma, &mu, &phi, &grad);
      std::printf("representation %zu %zu %d %.3e %.3e\n", n, phi.size(), p, error_of(phi, S, D), error_of(flat(grad), gS, gD));
      int equal = 0, count = 0;
      const std::vector<double> zero_s(S.size(), 0.0), zero_g(gS.size(), 0.0);
      for (int layers = 1; layers < 4; ++layers)
        for (int outs = 1; outs < 4; ++outs) {
          if (layers == 3 && outs == 3) continue;          // the full call, above
          std::vector<double> phi2, phi3;
          std::vector<V3> grad2, grad3;
          field->execute_representation(layers & 1 ? &sigma : nullptr, layers & 2 ? &mu : nullptr, outs & 1 ? &phi2 : nullptr, outs & 2 ? &grad2 : nullptr);
          // the same call with a zero vector for the missing layer, both outputs
          field->execute_representation(layers & 1 ? &sigma : &none, layers & 2 ? &mu : &none, &phi3, &grad3);
          const std::vector<double>&s = layers & 1 ? S : zero_s, &d = layers & 2 ? D : zero_s, &gs = layers & 1 ? gS : zero_g, &gd = layers & 2 ? gD : zero_g;
          if (outs & 1) { ++count; equal += layers == 3 ? same(phi2, phi) : error_of(phi2, phi3, zero_s) <= 1e-12 && error_of(phi2, s, d) <= 1e-11; } else equal -= !phi2.empty();
          if (outs & 2) { ++count; equal += layers == 3 ? same(grad2, grad) : error_of(flat(grad2), flat(grad3), zero_g) <= 1e-12 && error_of(flat(grad2), gs, gd) <= 1e-11; } else equal -= !grad2.empty();
        }
      std::printf("subsets %d %d %d\n", p, equal, count);
      if (p == 12) {
        std::printf("gradient %zu %zu %d\n", n, grad.size(), p);
        for (const auto& x : grad) std::printf("%.17g %.17g %.17g\n", x[0], x[1], x[2]);
      }
    }
  } catch (const fmmbem::Error& e) {
    std::printf("error %d %s\n", e.status, e.what());
    return 2;
  }
  return 0;
}
