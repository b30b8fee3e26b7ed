// fmmbem/Direct.hpp -- the device Direct sum for the adapter's kernel classes: r_i = sum_j K(t_i, s_j) c_j over ALL sources, summed on
// the device where the entries are made (fmmbem_direct_*, include/fmmbem.h) instead of entry by entry on the host.
//
//     fmmbem::DirectSum<Kernel> D(K, sources);          // uploads the panels once
//     results = D.matvec(charges, targets);             // Direct::matvec(K, s, c, t, r) of include/Direct.hpp:236-247, r overwritten
//     results = D.matvec(charges);                      // the symmetric form (:291-302): targets = sources
//     fmmbem::direct_matvec(K, sources, charges, targets, results);   // one call, "+=" into results as Direct::matvec does
//     D.gradient(charges, targets);                     // Laplace: the field gradient, D.hessian its derivative;  Stokes: D.pressure, D.velocity_gradient, D.stress
//
// A target's centre and BC are what count, as in FMM_plan(K, sources, targets, opts).  The order of addition is the library's fixed
// one (include/fmmbem.h), not the host loop's of compat/Direct.hpp: the two agree to rounding, not bit for bit, which is why the
// reference-named Direct::matvec keeps its own route and a caller opts in by name.
#pragma once
#include <array>
#include <cstring>
#include <vector>

#include "FMM_plan.hpp"

namespace fmmbem {

template <class Kernel>
class DirectSum {
 public:
  typedef Kernel kernel_type;
  typedef typename kernel_type::source_type source_type;
  typedef typename kernel_type::target_type target_type;
  typedef typename kernel_type::charge_type charge_type;
  typedef typename kernel_type::result_type result_type;

  DirectSum(const kernel_type& K, const std::vector<source_type>& sources, int device = 0) : n_(sources.size()) {
    std::vector<double> v(9 * n_);
    source_bc_.resize(n_);
    for (size_t i = 0; i < n_; ++i) {
      SingleOperators::vertices_of(sources[i], &v[9 * i]);
      source_bc_[i] = sources[i].BC == source_type::BC1;
    }
    fmmbem_options o;
    fmmbem_options_default(&o);
    FMMOptions none;
    KernelBinding<Kernel>::fill(K, none, o);
    o.device = device;
    mu_ = o.mu;
    check(fmmbem_direct_create(&o, n_, v.data(), &h_));
  }
  ~DirectSum() { fmmbem_direct_destroy(h_); }
  DirectSum(const DirectSum&) = delete;
  DirectSum& operator=(const DirectSum&) = delete;

  std::vector<result_type> matvec(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    std::vector<double> pts(3 * targets.size());
    std::vector<uint8_t> bc(targets.size());
    for (size_t i = 0; i < targets.size(); ++i) {
      for (int c = 0; c < 3; ++c) pts[3 * i + c] = targets[i].center[c];
      bc[i] = targets[i].BC == target_type::BC1;
    }
    std::vector<result_type> results(targets.size());
    check(fmmbem_direct_apply(h_, targets.size(), pts.data(), bc.data(), KernelBinding<Kernel>::in(charges), KernelBinding<Kernel>::out(results)));
    return results;
  }
  // targets = sources: the panels' own centres as the device computed them, the panels' own flags
  std::vector<result_type> matvec(const std::vector<charge_type>& charges) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    std::vector<result_type> results(n_);
    check(fmmbem_direct_apply(h_, n_, nullptr, source_bc_.data(), KernelBinding<Kernel>::in(charges), KernelBinding<Kernel>::out(results)));
    return results;
  }

  // Not in the reference: the field quantities at the targets' centres over ALL sources (fmmbem_direct_gradient / _hessian /
  // _pressure / _velocity_gradient) -- the sums that FMM_plan's execute_gradient, execute_pressure, execute_velocity_gradient and execute_stress
  // approximate, with their return types and scaling.  gradient: Laplace kernels, the target's BC picks gamma; pressure,
  // velocity_gradient, stress: Stokes kernels, the targets' BCs are not read.  The other kernel's methods throw
  // Error(FMMBEM_ERR_UNSUPPORTED), the library's refusal.
  std::vector<Vec<3, double>> gradient(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    std::vector<uint8_t> bc;
    const std::vector<double> pts = points_of(targets, &bc);
    std::vector<Vec<3, double>> results(targets.size());
    check(fmmbem_direct_gradient(h_, targets.size(), pts.data(), bc.data(), KernelBinding<Kernel>::in(charges), results.empty() ? nullptr : results.data()->data()));
    return results;
  }
  // the Hessian of the Laplace field (fmmbem_direct_hessian): H[a][b] row-major, the target's BC picks eta; Laplace kernels
  std::vector<std::array<double, 9>> hessian(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    std::vector<uint8_t> bc;
    const std::vector<double> pts = points_of(targets, &bc);
    std::vector<std::array<double, 9>> results(targets.size());
    check(fmmbem_direct_hessian(h_, targets.size(), pts.data(), bc.data(), KernelBinding<Kernel>::in(charges), results.empty() ? nullptr : results.data()->data()));
    return results;
  }
  std::vector<double> pressure(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    const std::vector<double> pts = points_of(targets, nullptr);
    std::vector<double> results(targets.size());
    check(fmmbem_direct_pressure(h_, targets.size(), pts.data(), KernelBinding<Kernel>::in(charges), results.data()));
    return results;
  }
  std::vector<std::array<double, 9>> velocity_gradient(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    if (charges.size() != n_) throw Error(FMMBEM_ERR_INVALID, "charges.size() != number of sources");
    const std::vector<double> pts = points_of(targets, nullptr);
    std::vector<std::array<double, 9>> results(targets.size());
    check(fmmbem_direct_velocity_gradient(h_, targets.size(), pts.data(), KernelBinding<Kernel>::in(charges), results.empty() ? nullptr : results.data()->data()));
    return results;
  }
  // sigma[k][m] = -q delta_km + mu (G[k][m] + G[m][k]), composed as FMM_plan::execute_stress composes it
  std::vector<std::array<double, 9>> stress(const std::vector<charge_type>& charges, const std::vector<target_type>& targets) {
    const std::vector<double> q = pressure(charges, targets);
    std::vector<std::array<double, 9>> g = velocity_gradient(charges, targets);
    for (size_t i = 0; i < g.size(); ++i) {
      std::array<double, 9> s;
      for (int k = 0; k < 3; ++k)
        for (int m = 0; m < 3; ++m) s[3 * k + m] = -q[i] * (k == m ? 1.0 : 0.0) + mu_ * (g[i][3 * k + m] + g[i][3 * m + k]);
      g[i] = s;
    }
    return g;
  }

  size_t size() const { return n_; }
  fmmbem_direct* handle() { return h_; }
  static int chunk() { return fmmbem_direct_chunk(); }

 private:
  // the targets' centres as n x 3 doubles; bc non-null: their flags too
  static std::vector<double> points_of(const std::vector<target_type>& targets, std::vector<uint8_t>* bc) {
    std::vector<double> pts(3 * targets.size());
    if (bc) bc->resize(targets.size());
    for (size_t i = 0; i < targets.size(); ++i) {
      for (int c = 0; c < 3; ++c) pts[3 * i + c] = targets[i].center[c];
      if (bc) (*bc)[i] = targets[i].BC == target_type::BC1;
    }
    return pts;
  }

  size_t n_;
  double mu_ = 1.0;                                   // the viscosity the handle was created with (stress)
  std::vector<uint8_t> source_bc_;
  fmmbem_direct* h_ = nullptr;
};

// Direct::matvec(K, sources, charges, targets, results) of include/Direct.hpp:276-289 on the device: results[i] += sum_j ...
template <class Kernel>
void direct_matvec(const Kernel& K, const std::vector<typename Kernel::source_type>& sources, const std::vector<typename Kernel::charge_type>& charges,
                   const std::vector<typename Kernel::target_type>& targets, std::vector<typename Kernel::result_type>& results, int device = 0) {
  if (results.size() != targets.size()) throw Error(FMMBEM_ERR_INVALID, "results.size() != targets.size()");
  if (sources.empty() || targets.empty()) return;
  DirectSum<Kernel> D(K, sources, device);
  const std::vector<typename Kernel::result_type> r = D.matvec(charges, targets);
  for (size_t i = 0; i < r.size(); ++i) results[i] += r[i];
}

}  // namespace fmmbem
