// The treecode evaluator through the header-only adapter, without a device: get_options(argc, argv) reads `-eval TREE`
// (FMMOptions.hpp:85-94), FMMOptions::c_evaluator() maps it to FMMBEM_EVAL_TREECODE, a host-only plan created with that value
// holds the FMM plan's lists, and a StokesSphericalBEM plan with it surfaces the library's FMMBEM_ERR_UNSUPPORTED as fmmbem::Error.
// usage: treecode_options <recursions> [reference-style flags]
// prints:  evaluator <c_evaluator> <c_evaluator with local_evaluation> <... with block_diagonal>
//          host_plan <status> <m2l_pairs> <p2p_pairs> <m2l_pairs of the FMM plan> <p2p_pairs of the FMM plan>
//          stokes <status thrown, or 0>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmmbem/FMM_plan.hpp"

static int host_counts(int evaluator, size_t n, const std::vector<double>& v, long long* m2l, long long* p2p) {
  fmmbem_options o;
  fmmbem_options_default(&o);
  o.host_only = 1;
  o.ncrit = 8;                                         // small leaves: long-range pairs already on a sphere of 128 panels
  o.evaluator = evaluator;
  fmmbem_plan* plan = nullptr;
  const int rc = fmmbem_plan_create(&o, n, v.data(), nullptr, &plan);
  if (rc != FMMBEM_OK) return rc;
  fmmbem_stats st;
  const int rs = fmmbem_plan_stats(plan, &st);
  *m2l = (long long)st.m2l_pairs;
  *p2p = (long long)st.p2p_pairs;
  fmmbem_plan_destroy(plan);
  return rs;
}

int main(int argc, char** argv) {
  const int recursions = argc > 1 ? std::atoi(argv[1]) : 3;
  FMMOptions opts = get_options(argc, argv);
  FMMOptions local = opts, diag = opts;
  local.lazy_evaluation = false; local.local_evaluation = true;
  diag.lazy_evaluation = false; diag.block_diagonal = true;
  std::printf("evaluator %d %d %d\n", opts.c_evaluator(), local.c_evaluator(), diag.c_evaluator());

  size_t n = 0;
  fmmbem_mesh_unit_sphere(recursions, nullptr, &n);
  std::vector<double> v(9 * n);
  fmmbem_mesh_unit_sphere(recursions, v.data(), &n);
  long long m2l = -1, p2p = -1, m2l_fmm = -1, p2p_fmm = -1;
  const int rc = host_counts(opts.c_evaluator(), n, v, &m2l, &p2p);
  host_counts(FMMBEM_EVAL_FMM, n, v, &m2l_fmm, &p2p_fmm);
  std::printf("host_plan %d %lld %lld %lld %lld\n", rc, m2l, p2p, m2l_fmm, p2p_fmm);

  int thrown = 0;
  if (opts.c_evaluator() == FMMBEM_EVAL_TREECODE) try {      // refused before any device is touched
    typedef StokesSphericalBEM::point_type P;
    StokesSphericalBEM K(5, 4, 1e-3);
    std::vector<StokesSphericalBEM::source_type> panels;
    for (size_t i = 0; i < n; ++i)
      panels.push_back(StokesSphericalBEM::source_type(P(v[9 * i], v[9 * i + 1], v[9 * i + 2]), P(v[9 * i + 3], v[9 * i + 4], v[9 * i + 5]),
                                                       P(v[9 * i + 6], v[9 * i + 7], v[9 * i + 8])));
    FMM_plan<StokesSphericalBEM> plan(K, panels, opts);
  } catch (const fmmbem::Error& e) {
    thrown = e.status;
  }
  std::printf("stokes %d\n", thrown);
  return 0;
}
