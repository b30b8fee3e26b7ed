// direct.hip -- fmmbem_direct_* of include/fmmbem.h: the reference's Direct::matvec (include/Direct.hpp:232-302) as a device sum.
// A handle owns a DevicePlan that holds ONLY the source panels, in the caller's order -- built the way ops.hip builds its two-box
// plan, with the panels' derived geometry from panel_setup_kernel (identity permutation), so centroids, normals, areas and quadrature
// points carry the bits a plan's carry.  No tree, no permutation, no matrix.  The sum itself is kernels_direct.hip.
// fmmbem_direct_{gradient,pressure,velocity_gradient}: the field quantities at points summed the same way, over one routine.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/fmmbem.h"
#include "device_allocs.hpp"
#include "device_launch.hpp"
#include "host_plan.hpp"
#include "status.hpp"

using namespace fmmbem;

namespace {

bool all_finite(const double* v, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

constexpr size_t kPartCap = (size_t)1 << 25;           // doubles of partial sums one launch may need (256 MB): more targets go in slabs

}  // namespace

struct fmmbem_direct {
  int device = 0;
  int64_t n = 0;
  DevicePlan d{};                                      // the source panels and the rules; nothing else is set
  DeviceAllocs mem;
  hipStream_t stream = nullptr;                        // the host form's stream
  double* part = nullptr;                              // [chunk][target][dof] partial sums, grown on demand
  size_t part_cap = 0;                                 // doubles
  ~fmmbem_direct() {
    DeviceGuard g(device);
    mem.free_all();
    if (part) (void)hipFree(part);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <class T>
  int alloc(size_t count, T** out) { return mem.alloc(count, out, false); }
  template <class T>
  int upload(const std::vector<T>& v, const T** out) { return mem.upload(v, out); }
  int init(const fmmbem_options& o, const QuadRule& rule, const QuadRule& fine, const double* vertices);
  int ensure_part(size_t doubles);
  // q null: the operator, width = d.dof; else the field quantity *q at points, width = direct_field_width(*q)
  int apply(size_t m, int width, const FieldQuantity* q, const double* d_pts, const uint8_t* d_bc, const double* d_x, double* d_y,
            hipStream_t s);
};

int fmmbem_direct::init(const fmmbem_options& o, const QuadRule& rule, const QuadRule& fine, const double* vertices) {
  const bool stokes = o.kernel == FMMBEM_KERNEL_STOKES_BEM;
  const size_t nn = (size_t)n;
  d.n = n; d.nq = rule.n; d.kernel = o.kernel; d.dof = stokes ? 3 : 1; d.mu = stokes ? o.mu : 1.0;
  for (int q = 0; q < rule.n; ++q) d.qw[q] = rule.w[q];
  HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  if (stokes) {
    d.nqf = fine.n;
    std::vector<double> qf((size_t)fine.n * 4);
    for (int q = 0; q < fine.n; ++q) { for (int k = 0; k < 3; ++k) qf[4 * q + k] = fine.pts[q][k]; qf[4 * q + 3] = fine.w[q]; }
    TRY(upload(qf, &d.qf));
  }
  double *cx, *cy, *cz, *nx, *ny, *nz, *ar, *qd, *vt;
  TRY(alloc(nn, &cx)); TRY(alloc(nn, &cy)); TRY(alloc(nn, &cz));
  TRY(alloc(nn, &nx)); TRY(alloc(nn, &ny)); TRY(alloc(nn, &nz));
  TRY(alloc(nn, &ar)); TRY(alloc(nn * 3 * rule.n, &qd)); TRY(alloc(nn * 9, &vt));
  {
    // sources carry no flags (the target's picks the operator): bc stays zero; perm is the identity
    std::vector<uint8_t> bc(nn, 0);
    std::vector<uint32_t> perm(nn);
    std::iota(perm.begin(), perm.end(), 0u);
    TRY(upload(bc, &d.bc)); TRY(upload(perm, &d.perm));
  }
  std::vector<double> pts((size_t)rule.n * 3);
  for (int q = 0; q < rule.n; ++q) for (int k = 0; k < 3; ++k) pts[3 * q + k] = rule.pts[q][k];
  Scratch sc;
  const double *d_pts = nullptr, *v_orig = nullptr;
  TRY(sc.up(pts.data(), pts.size(), &d_pts));
  TRY(sc.up(vertices, 9 * nn, &v_orig));
  HIP_TRY(launch_panel_setup(n, d.perm, v_orig, rule.n, d_pts, cx, cy, cz, nx, ny, nz, ar, qd, vt, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  d.cx = cx; d.cy = cy; d.cz = cz; d.nx = nx; d.ny = ny; d.nz = nz; d.area = ar; d.quad = qd; d.vert = vt;
  return FMMBEM_OK;
}

int fmmbem_direct::ensure_part(size_t doubles) {
  if (doubles <= part_cap) return FMMBEM_OK;
  if (part) (void)hipFree(part);                       // (waits for the launches that still read it)
  part = nullptr; part_cap = 0;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, doubles * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(FMMBEM_ERR_ALLOC, std::string("Direct: partial-sum buffer: ") + hipGetErrorString(e));
  }
  part = static_cast<double*>(p); part_cap = doubles;
  return FMMBEM_OK;
}

int fmmbem_direct::apply(size_t m, int width, const FieldQuantity* q, const double* d_pts, const uint8_t* d_bc, const double* d_x, double* d_y,
                         hipStream_t s) {
  const size_t per_target = (size_t)direct_chunks(n) * (size_t)width;
  size_t slab = m;
  if (per_target * m > kPartCap) slab = std::max<size_t>(256, kPartCap / per_target / 256 * 256);
  TRY(ensure_part(per_target * std::min(m, slab)));
  for (size_t off = 0; off < m; off += slab) {
    const size_t mm = std::min(slab, m - off);
    if (q) {
      HIP_TRY(launch_direct_field(*q, d, (int64_t)mm, d_pts + 3 * off, d_bc ? d_bc + off : nullptr, d_x, part, d_y + off * width, s));
      continue;
    }
    const double *tx = d_pts ? d_pts + 3 * off : d.cx + off, *ty = d_pts ? tx + 1 : d.cy + off, *tz = d_pts ? tx + 2 : d.cz + off;
    HIP_TRY(launch_direct(d, (int64_t)mm, tx, ty, tz, d_pts ? 3 : 1, d_bc ? d_bc + off : nullptr, d_x, part, d_y + off * d.dof, s));
  }
  return FMMBEM_OK;
}

namespace {

// fmmbem_direct_{gradient,pressure,velocity_gradient,hessian}{,_device}: the checks in the header's order, then the sum.  host: the pointers
// are the caller's host arrays (the points are read, the result is copied back); else device pointers, asynchronous on s.
int direct_field(fmmbem_direct* direct, FieldQuantity q, bool host, size_t n_targets, const double* pts, const uint8_t* bc, const double* x,
                 double* out, hipStream_t s) {
  static const char* const kName[4] = {"gradient", "pressure", "velocity gradient", "Hessian"};
  const char* name = kName[(int)q];
  if (!direct || !pts || !x || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (n_targets == 0) return fail(FMMBEM_ERR_INVALID, std::string("Direct ") + name + ": no targets");
  const bool laplace = direct->d.dof == 1;
  if (q == FieldQuantity::Gradient && !laplace)
    return fail(FMMBEM_ERR_UNSUPPORTED, "Direct gradient: the gradient of the Laplace field needs a handle of the Laplace kernel (this one is Stokes: "
                                        "fmmbem_direct_velocity_gradient is its gradient)");
  if (q == FieldQuantity::Hessian && !laplace)
    return fail(FMMBEM_ERR_UNSUPPORTED, "Direct Hessian: the Hessian of the Laplace field needs a handle of the Laplace kernel (this one is Stokes: "
                                        "fmmbem_direct_velocity_gradient is its second-order quantity)");
  if (q != FieldQuantity::Gradient && q != FieldQuantity::Hessian && laplace)
    return fail(FMMBEM_ERR_UNSUPPORTED, std::string("Direct ") + name + ": the " + name + " of the single layer needs a handle of the Stokes kernel "
                                        "(this one is Laplace: fmmbem_direct_gradient is its gradient)");
  if (host && !all_finite(pts, 3 * n_targets)) return fail(FMMBEM_ERR_INVALID, std::string("Direct ") + name + ": a target point is not finite");
  DeviceGuard guard(direct->device);
  HIP_TRY(guard.err);
  const int width = direct_field_width(q);
  if (!host) return direct->apply(n_targets, width, &q, pts, bc, x, out, s);
  Scratch sc;
  const double *d_pts = nullptr, *d_x = nullptr;
  const uint8_t* d_bc = nullptr;
  double* d_out = nullptr;
  TRY(sc.up(pts, 3 * n_targets, &d_pts));
  if (bc) TRY(sc.up(bc, n_targets, &d_bc));
  TRY(sc.up(x, (size_t)direct->n * (size_t)direct->d.dof, &d_x));
  TRY(sc.alloc(n_targets * width, &d_out));
  TRY(direct->apply(n_targets, width, &q, d_pts, d_bc, d_x, d_out, direct->stream));
  HIP_TRY(hipStreamSynchronize(direct->stream));
  HIP_TRY(hipMemcpy(out, d_out, n_targets * width * sizeof(double), hipMemcpyDeviceToHost));
  return FMMBEM_OK;
}

}  // namespace

extern "C" {

int fmmbem_direct_gradient(fmmbem_direct* direct, size_t n_targets, const double* target_points, const uint8_t* target_bc, const double* x,
                           double* g) {
  return direct_field(direct, FieldQuantity::Gradient, true, n_targets, target_points, target_bc, x, g, nullptr);
}
int fmmbem_direct_gradient_device(fmmbem_direct* direct, size_t n_targets, const double* d_target_points, const uint8_t* d_target_bc,
                                  const double* d_x, double* d_g, void* stream) {
  return direct_field(direct, FieldQuantity::Gradient, false, n_targets, d_target_points, d_target_bc, d_x, d_g, static_cast<hipStream_t>(stream));
}
int fmmbem_direct_hessian(fmmbem_direct* direct, size_t n_targets, const double* target_points, const uint8_t* target_bc, const double* x,
                          double* H) {
  return direct_field(direct, FieldQuantity::Hessian, true, n_targets, target_points, target_bc, x, H, nullptr);
}
int fmmbem_direct_hessian_device(fmmbem_direct* direct, size_t n_targets, const double* d_target_points, const uint8_t* d_target_bc,
                                 const double* d_x, double* d_H, void* stream) {
  return direct_field(direct, FieldQuantity::Hessian, false, n_targets, d_target_points, d_target_bc, d_x, d_H, static_cast<hipStream_t>(stream));
}
int fmmbem_direct_pressure(fmmbem_direct* direct, size_t n_targets, const double* target_points, const double* x, double* q) {
  return direct_field(direct, FieldQuantity::Pressure, true, n_targets, target_points, nullptr, x, q, nullptr);
}
int fmmbem_direct_pressure_device(fmmbem_direct* direct, size_t n_targets, const double* d_target_points, const double* d_x, double* d_q,
                                  void* stream) {
  return direct_field(direct, FieldQuantity::Pressure, false, n_targets, d_target_points, nullptr, d_x, d_q, static_cast<hipStream_t>(stream));
}
int fmmbem_direct_velocity_gradient(fmmbem_direct* direct, size_t n_targets, const double* target_points, const double* x, double* G) {
  return direct_field(direct, FieldQuantity::VelocityGradient, true, n_targets, target_points, nullptr, x, G, nullptr);
}
int fmmbem_direct_velocity_gradient_device(fmmbem_direct* direct, size_t n_targets, const double* d_target_points, const double* d_x,
                                           double* d_G, void* stream) {
  return direct_field(direct, FieldQuantity::VelocityGradient, false, n_targets, d_target_points, nullptr, d_x, d_G, static_cast<hipStream_t>(stream));
}

int fmmbem_direct_create(const fmmbem_options* opts, size_t n_sources, const double* source_vertices, fmmbem_direct** out) {
  if (out) *out = nullptr;
  if (!opts || !source_vertices || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (opts->kernel != FMMBEM_KERNEL_LAPLACE_BEM && opts->kernel != FMMBEM_KERNEL_STOKES_BEM)
    return fail(FMMBEM_ERR_UNSUPPORTED, "unknown kernel id");
  if (n_sources == 0) return fail(FMMBEM_ERR_INVALID, "Direct: no sources");
  if (direct_chunks((int64_t)n_sources) > 65535) return fail(FMMBEM_ERR_INVALID, "Direct: too many sources (65535 chunks at most)");
  const bool stokes = opts->kernel == FMMBEM_KERNEL_STOKES_BEM;
  QuadRule rule, fine;
  if (!quad_rule(opts->quad_k, rule)) return fail(FMMBEM_ERR_INVALID, "invalid quadrature key (valid: 1 3 4 7 13 17 19 25 79)");
  if (stokes) {
    if (!quad_rule(opts->quad_k_fine, fine)) return fail(FMMBEM_ERR_INVALID, "invalid K_fine (valid: 1 3 4 7 13 17 19 25 79)");
    if (!(opts->mu > 0)) return fail(FMMBEM_ERR_INVALID, "Stokes: viscosity mu must be positive");
  }
  if (!all_finite(source_vertices, 9 * n_sources)) return fail(FMMBEM_ERR_INVALID, "Direct: a source vertex is not finite");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMMBEM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU execution path)");
  if (opts->device < 0 || opts->device >= ndev) return fail(FMMBEM_ERR_INVALID, "device ordinal out of range");
  std::unique_ptr<fmmbem_direct> h(new (std::nothrow) fmmbem_direct);
  if (!h) return fail(FMMBEM_ERR_ALLOC, "Direct handle");
  h->device = opts->device; h->n = (int64_t)n_sources;
  DeviceGuard guard(h->device);
  HIP_TRY(guard.err);
  try {
    TRY(h->init(*opts, rule, fine, source_vertices));
  } catch (const std::bad_alloc&) {
    return fail(FMMBEM_ERR_ALLOC, "host allocation failed");
  }
  *out = h.release();
  return FMMBEM_OK;
}

int fmmbem_direct_apply_device(fmmbem_direct* direct, size_t n_targets, const double* d_target_points, const uint8_t* d_target_bc,
                               const double* d_x, double* d_y, void* stream) {
  if (!direct || !d_x || !d_y) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (n_targets == 0) return fail(FMMBEM_ERR_INVALID, "Direct: no targets");
  if (!d_target_points && n_targets != (size_t)direct->n)
    return fail(FMMBEM_ERR_INVALID, "Direct: the symmetric form (no target points) takes n_targets = n_sources");
  DeviceGuard guard(direct->device);
  HIP_TRY(guard.err);
  return direct->apply(n_targets, direct->d.dof, nullptr, d_target_points, d_target_bc, d_x, d_y, static_cast<hipStream_t>(stream));
}

int fmmbem_direct_apply(fmmbem_direct* direct, size_t n_targets, const double* target_points, const uint8_t* target_bc, const double* x,
                        double* y) {
  if (!direct || !x || !y) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (n_targets == 0) return fail(FMMBEM_ERR_INVALID, "Direct: no targets");
  if (!target_points && n_targets != (size_t)direct->n)
    return fail(FMMBEM_ERR_INVALID, "Direct: the symmetric form (no target points) takes n_targets = n_sources");
  if (target_points && !all_finite(target_points, 3 * n_targets)) return fail(FMMBEM_ERR_INVALID, "Direct: a target point is not finite");
  DeviceGuard guard(direct->device);
  HIP_TRY(guard.err);
  const size_t dof = (size_t)direct->d.dof;
  Scratch sc;
  const double *d_pts = nullptr, *d_x = nullptr;
  const uint8_t* d_bc = nullptr;
  double* d_y = nullptr;
  if (target_points) TRY(sc.up(target_points, 3 * n_targets, &d_pts));
  if (target_bc) TRY(sc.up(target_bc, n_targets, &d_bc));
  TRY(sc.up(x, (size_t)direct->n * dof, &d_x));
  TRY(sc.alloc(n_targets * dof, &d_y));
  TRY(direct->apply(n_targets, direct->d.dof, nullptr, d_pts, d_bc, d_x, d_y, direct->stream));
  HIP_TRY(hipStreamSynchronize(direct->stream));
  HIP_TRY(hipMemcpy(y, d_y, n_targets * dof * sizeof(double), hipMemcpyDeviceToHost));
  return FMMBEM_OK;
}

int fmmbem_direct_chunk(void) { return direct_chunk(); }

void fmmbem_direct_destroy(fmmbem_direct* direct) { delete direct; }

}  // extern "C"
