// plan.hip -- implementation of the C ABI declared in include/fmmbem.h.
// Host orchestration only: builds the HostPlan, tabulates the translation operators, uploads
// everything once, and sequences the gfx950 kernels of kernels_near.hip / kernels_far.hip on a HIP
// stream.  There is NO CPU execution path: without a device, execute returns FMMBEM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/fmmbem.h"
#include "blockinv.hpp"
#include "device_allocs.hpp"
#include "device_launch.hpp"
#include "host_plan.hpp"
#include "host_tables.hpp"
#include "launch_choice.hpp"
#include "m2l_layout.hpp"
#include "m2l_rot.hpp"
#include "plan_layout.hpp"
#include "shift_ops.hpp"
#include "status.hpp"

using namespace fmmbem;
using namespace fmmbem::tables;

namespace {
thread_local std::string g_last_error;
}
namespace fmmbem {
int fail(int code, const std::string& msg) {          // status.hpp; also used by mesh_io.cpp
  g_last_error = msg;
  return code;
}
struct SolverWs;                                      // krylov.hip
void solver_ws_destroy(SolverWs* ws);
int plan_solver_info(fmmbem_plan* plan, int* device, int64_t* unknowns, int* p_max, SolverWs*** slot);
size_t plan_unknowns(const fmmbem_plan* plan);
bool plan_block_inverse_built(const fmmbem_plan* plan);
}  // namespace fmmbem

namespace {

#define DEVICE_SCOPE(dev)        \
  DeviceGuard device_guard_(dev); \
  HIP_TRY(device_guard_.err)

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// What one direction of the tree, M2M up or L2L down, reads on the device, and its level launches
struct ShiftSide {
  const int *rsrc = nullptr, *rcls = nullptr, *rtgt = nullptr; // the pairs (source box, class, target box) of all launches, launch after launch
  const int* ritem = nullptr;                                  // the rotation kernel's items: pair ranges of at most one pass
  const int* unit_ptr = nullptr;                               // up: first pair of every parent, per launch; down (a pair is a unit): null
  const double *rec = nullptr, *stream = nullptr;              // class records; the rotation kernel's constant stream, all orders
  const double *sl_class = nullptr, *sl_rc = nullptr, *sl_xc = nullptr;       // one pair per wavefront: class table, and the lanes'
  const int32_t *sl_rs = nullptr, *sl_xs = nullptr;                           // four tables, all orders
  std::vector<ShiftOpDev> ops;                                 // the sparse operators, index p - 1
  std::vector<std::pair<int, int>> launch;                     // (first, count) per level
  std::vector<ShiftRot> rot;                                   // the same launches for the rotation and wavefront kernels
};

// The device side of what depends on the GEOMETRY and the options only: written once by geometry creation (to_device_near,
// to_device_far, and the options in fmmbem_plan_create*), never changed afterwards.  A plan reads it through a const reference.
struct PlanGeometry {
  fmmbem_options opts{};                                       // as given to the creation: what same_geometry_options compares
  DevicePlan gd;                                               // the geometry's fields of a plan's DevicePlan (gd.n: the panel count)
  ShiftSide up, down;                                          // M2M / L2L
  std::vector<std::pair<int, int>> m2m_shared_launch;          // sharded upward pass: parents spanning shards (pairs and items in `up`)
  std::vector<ShiftRot> m2m_shared_rot;
  bool shift_lanes = true;                                     // this and shift_lanes_max, shift_rot_min, shift_rot: the switches of the tree-pass rule (launch_choice.hpp shift_form)
  int shift_lanes_max = -1;                                    // FMMBEM_SHIFT_LANES_MAX
  size_t sl_rot_off[kShiftLanesPmax + 1] = {}, sl_ax_off[kShiftLanesPmax + 1] = {};     // into a side's sl_rc, sl_rs / sl_xc, sl_xs, by order
  int shift_stream_off[12] = {};                               // into a side's stream, index p - 1
  int shift_rot_min = 2048;                                    // boxes on a tree level from which the rotation kernels take it
  bool shift_rot = true;
  bool split_upward = false;                                   // P2M/M2M sharded by owner, multipoles all-gathered by the caller
  // L2P's last store delivers the result, y[perm[i]] = y_tree[i] + far field, and no scatter kernel runs: a Laplace plan on its own
  // panels, one shard, whose L2P groups cover every row (decided once, to_device_far).  FMMBEM_L2P_SCATTER=0 keeps the separate
  // kernel (read per execute, for A/B runs).  The same single rounded add either way: the same bits.
  bool l2p_scatter = false;
  M2PWork m2p;                                                 // treecode plans (FMMBEM_EVAL_TREECODE): the far field's work, else empty
  // sizes of the stored near blocks (allocated per plan, to_device_bc_begin)
  int64_t near_total_doubles = 0, sym_total_doubles = 0;
  int64_t near_bytes = 0;
  // hybrid near field (fmmbem_options.near_stream_fraction < 1): which leaves keep no matrix; host copies of the block offsets
  bool hybrid = false;
  std::vector<uint8_t> near_rec_host;                          // [leaf] 1 = recomputed
  std::vector<int64_t> near_off_host, sym_off_host;            // [leaf] offsets of the stored blocks (introspection)
  int64_t near_recomputed_pairs = 0;
  // float near field (fmmbem_options.near_f32_max_p): floats of the copy (0: not active on this geometry; the copy itself is
  // allocated and filled per plan in to_device_bc_begin)
  int64_t near_f32_floats = 0;
  int64_t n_classes = 0;
  // which M2L an execute at order p takes: the rotation kernel for the orders it is instantiated for (p <= 12), the double-sum
  // kernels above; FMMBEM_M2L_ROT=0: the double sum at every order (A/B runs, tools/m2l_ab.py)
  int rot_max = kRotPmax;
  bool use_rot(int p) const { return p <= rot_max && m2l_rot_supported(p); }
};

// What a plan holds that depends on the GEOMETRY and the options only -- the octree, the permutation, every pair list, the work
// items and run descriptors, the panels' points, the operator tables, the launch lists -- on the host and in HBM.  Plans of the
// same panels that differ in the boundary-condition flags alone (the drivers' right-hand-side plan beside the operator,
// examples/LaplaceBEM.cpp:209-232, StokesBEM.cpp:266-270) share ONE of these through a reference count (fmmbem_plan_create_like,
// and fmmbem_plan_create itself when it recognises a geometry that is still alive); freed with the last plan that points to it.
struct PlanShared {
  HostPlan hp;
  PlanGeometry geo;
  DeviceAllocs allocs;                                         // (freed with the last plan, on the device they name)
  uint64_t fingerprint[2] = {0, 0};                            // of the vertex bytes (original order), 0 0: not taken
};

// The flag side of a plan's DevicePlan: what to_device_bc_begin / to_device_bc_end / build_side_lists decide and allocate, with
// the types of the DevicePlan fields of the same names.  compose_d() is the only place a plan's d is put together.
struct FlagFields {
  const uint8_t* bc = nullptr;
  int n_act = 0, nslots = 2;
  int act[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int stokes_velocity_targets = 1, stokes_traction_targets = 0;
  double *near_val = nullptr, *near_sym = nullptr;
  float* near_f32 = nullptr;
  double *ys = nullptr, *xt4 = nullptr;
  double2 *M = nullptr, *L = nullptr, *Mh = nullptr;
  double *xt = nullptr, *yt = nullptr;
  const double2 *p2m_tab = nullptr, *p2m_tab_g = nullptr;
  int64_t p2m_tab_row0 = 0;
  const int64_t* side_ptr = nullptr;
  const int* side_col = nullptr;
  const double* side_val = nullptr;
  const int4* side_items = nullptr;  int side_nitems = 0;
};

struct fmmbem_plan {
  fmmbem_options opts{};
  const std::shared_ptr<PlanShared> shared;
  HostPlan& hp;                                                // = shared->hp
  const PlanGeometry& g;                                       // = shared->geo
  FlagFields fd;
  DevicePlan d;                                                // = g.gd + fd (compose_d)
  const DevicePlan* d_dev = nullptr;                           // copy of d in device memory
  bool on_device = false;
  bool has_bc[2] = {false, false};                             // boundary-condition flags present among THIS plan's panels
  DeviceAllocs allocs;                                         // what this plan alone owns: everything that depends on the flags
  DeviceAllocs* mem = &allocs;                                 // where upload() / alloc() record: shared->allocs (geometry creation) or allocs
  // every plan is built on a shared block: a new one (fmmbem_plan_create*), a live one (like()), a shard's (the handle of a
  // multi-device plan).  Never copied: what a plan owns has one owner.
  explicit fmmbem_plan(std::shared_ptr<PlanShared> sh) : shared(std::move(sh)), hp(shared->hp), g(shared->geo) {}
  fmmbem_plan(const fmmbem_plan&) = delete;
  // A plan over SEVERAL devices of one process (fmmbem_options.n_devices > 1): this handle then owns one shard plan per device and
  // does the copies between them itself (MultiDevice, further down); everything else in this struct belongs to single-device plans
  std::shared_ptr<struct MultiDevice> multi;
  // hipGraphs of the launch chain between the gather and the delivery of a matvec (those two take the caller's pointers),
  // one per (region of the execute, order p, exchange buffer): captured on own_stream the SECOND time a region runs at an
  // order (the first run goes out launch by launch, so that every one-time initialisation inside the launchers has happened),
  // then replayed on the caller's stream.  Off unless fmmbem_plan_set_graphs / FMMBEM_GRAPH=1: on this runtime dependent
  // launches already run back to back on the device (profiles/r03b), what a graph saves is host time per matvec.
  struct GraphEntry { int region, p; const void* buf; int runs; hipGraphExec_t exec; };
  // a region: the upward half, or what the rest of an execute holds -- the downward half (else a whole execute), the near field
  // already run (near_split), the near field alone, L2P's folded store, the combined near-field / P2M launch
  enum : int { kRegionUpward = 1, kRegionDownward = 2, kRegionNearDone = 4, kRegionNearOnly = 8, kRegionFold = 16, kRegionFused = 32 };
  std::vector<GraphEntry> graphs;
  bool use_graphs = false;
  // The treecode evaluator: an FMM plan up to and including M2M; the far field is then ONE stage, M2P from the multipoles into
  // y_tree (launch_m2p on g.m2p), and the ordinary scatter delivers.  Of the FMM path's shortcuts it takes none that look past
  // M2M: not L2P's folded scatter (l2p_delivers), not mh_prep or the rotation items (nothing reads Mh).  It also leaves the
  // combined near-field / P2M launch alone and runs the two launches: the same M bit for bit, and the treecode's critical path is
  // the M2P stage, not the near field's drain.
  bool treecode() const { return opts.evaluator == FMMBEM_EVAL_TREECODE; }
  // Whole: a matvec; Upward: the first half of a split execute (gather, P2M, M2M of owned boxes, pack -> xbuf); Downward: the
  // rest (xbuf = the gathered multipoles); NearSplit: the near field of a split execute, between the two
  enum class Phase { Whole, Upward, Downward, NearSplit };
  enum class Stage { Gather, Spmv, Scatter, P2M, M2M, Mh, M2L, L2L, L2P };          // the order fmmbem_plan_stats reads
  // Begin / end events around a stage (a kernel, or a level sequence) on its stream; by default none (timing off; a batch's far
  // chains).  An event record is a packet of its own between two kernels (~5 us each on this part: a fully instrumented matvec is
  // 85 us longer than a bare one), so a throughput measurement brackets the one kernel it needs (mode 2: the near field) alone.
  struct StageMarks {
    int mode = 0;                                              // fmmbem_plan::timing
    hipEvent_t* set = nullptr;                                 // this execute's kStages (begin, end) pairs of the ring
    unsigned mask = 0;                                         // stages recorded
    bool rec(Stage i) const { return mode == 1 || (mode == 2 && i == Stage::Spmv); }
    hipError_t begin(Stage i, hipStream_t st) { return rec(i) ? hipEventRecord(set[2 * (int)i], st) : hipSuccess; }
    hipError_t end(Stage i, hipStream_t st) {
      if (rec(i)) mask |= 1u << (int)i;
      return rec(i) ? hipEventRecord(set[2 * (int)i + 1], st) : hipSuccess;
    }
  };
  // the launchers of one stage on the DevicePlan given (the plan's d; a batch: vector j's view of it)
  enum class ShiftDir { Up, UpShared, Down };                  // M2M of the own boxes, of the parents spanning shards; L2L
  int shift_pass(const DevicePlan& dv, int p, ShiftDir dir, hipStream_t s) const;
  template <class Launch> int p2m_targets(const DevicePlan& dv, Launch&& launch) const;
  int p2m(const DevicePlan& dv, int p, StageMarks& tm, hipStream_t s) const;
  enum class L2PTo { YTree, Perm, Caller };                    // add into y_tree; store y_out[perm[i]]; nothing here (a capture: the caller's pointer comes after)
  int l2p(const DevicePlan& dv, int p, double* y_out, hipStream_t s) const;
  int far_chain(const DevicePlan& dv, const DevicePlan* dv_dev, int p, bool m2m_own, const double* xch, L2PTo to, double* y_out,
                StageMarks& tm, hipStream_t s) const;
  int deliver(const DevicePlan& dv, double* d_y, bool fold, hipStream_t s) const;
  size_t x_doubles() const { return (size_t)(targets ? hp.n_src : hp.n) * (opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1); }      // a target plan: x over the panels,
  size_t y_doubles() const { return (size_t)(targets ? hp.n_targets : hp.n) * (opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1); }  // y over the targets
  unsigned pending_mask = 0;                                   // stages recorded by the upward half of a split execute
  bool pending_near = false;                                   // split execute: the near field already ran (fmmbem_plan_near_split_device)
  bool result_slices = false;                                  // execute delivers the owned rows in tree order (fmmbem_plan_set_result_slices)
  bool l2p_delivers(bool near_only, Phase phase) const {       // (PlanGeometry::l2p_scatter)
    if (!g.l2p_scatter || result_slices || near_only || phase != Phase::Whole || treecode()) return false;   // a treecode runs no L2P
    return sw::l2p_scatter();
  }
  int64_t* d_cut = nullptr;                                    // tree-order row cuts of all shards, on the device
  int64_t near_side_entries = 0;                               // matrix-free plans: listed near-regime pairs (12 bytes each)
  int last_near_f32 = 0;                                       // float near field: what the last execute streamed
  HybridStreams hyb;                                           // the recompute kernel and the listed entries run beside the streaming one
  int build_side_lists();
  double build_host_ms = 0, build_assemble_ms = 0;
  // execute state
  int timing = 0;                                              // 0 off, 1 events around every stage, 2 around the near-field kernel only
  int last_p = 0;
  static constexpr int kStages = 9, kRing = 64;                // gather spmv scatter p2m m2m mh m2l l2l l2p
  std::vector<hipEvent_t> ev;                                  // kRing sets of 2*kStages events (begin, end)
  unsigned ev_mask[kRing] = {};                                // stages actually recorded in each set
  int64_t ev_count = 0;                                        // executes recorded since timing was enabled
  double *stage_x = nullptr, *stage_y = nullptr;               // device staging for host-pointer execute
  fmmbem::SolverWs* solver_ws = nullptr;                       // workspace of fmmbem_gmres* on this plan (krylov.hip), kept between solves
  hipStream_t own_stream = nullptr;
  // Exact block-Jacobi preconditioner of a BLOCK_DIAGONAL plan (fmmbem_plan_block_inverse_build; kernels_blockinv.hip): the
  // inverses of the leaves' self blocks in storage of their own -- near_val / near_sym stay what execute applies
  struct BlockInverse {
    bool built = false;
    BlockInvDev dev;
    int max_m = 0;                                             // unknowns of the largest leaf
    int64_t doubles = 0;                                       // of all inverses together
    double* stage = nullptr;                                   // device staging of the host-pointer apply: v, then z
    size_t stage_doubles = 0;
  };
  BlockInverse binv;
  void block_inverse_free() {
    for (void* p : {(void*)binv.dev.val, (void*)binv.dev.off, (void*)binv.dev.bad, (void*)binv.stage}) if (p) (void)hipFree(p);
    binv = BlockInverse{};
  }
  // Dual plans (fmmbem_plan_create_targets, fmmbem_plan_create_field): hp holds the source tree and the target tree as one plan
  // (HostPlan::build_targets); x has hp.n_src x dof entries, y hp.n_targets x dof.  Every source feeds every live expansion group
  // (the TARGET's flag picks the kernel).  Laplace: P2M runs once per live slot with the flags of all sources set to that slot's
  // (bc_all[slot]) and that slot's moment table.  Stokes: the single plan's P2M as it is -- it never reads a source's flag.
  bool targets = false;
  bool p2m_per_slot() const { return targets && opts.kernel != FMMBEM_KERNEL_STOKES_BEM; }
  bool zero_target_rows = false;                               // some target leaf has no near pair
  const uint8_t* bc_all[2] = {nullptr, nullptr};
  const double2* p2m_tab_slot[2] = {nullptr, nullptr};
  const uint32_t* d_target_point = nullptr;                    // given target -> distinct point (only when some coincide)
  double* y_points = nullptr;                                  // the result per distinct point (only when some coincide)
  double* stage_y_targets = nullptr;                           // device staging of y for host-pointer execute
  // Field quantities (fmmbem_plan_execute_gradient, _pressure, _velocity_gradient, _hessian; kField below): per quantity its width in doubles
  // per target row in tree order, per distinct point (only when some targets coincide) and per given target (the host form's
  // staging); each quantity's buffers are allocated at its first call
  struct FieldBuffers { double *tree = nullptr, *points = nullptr, *stage = nullptr; };
  FieldBuffers field[4];
  int field_refusal(FieldQuantity q, int p) const;
  int field_alloc(FieldQuantity q);
  int run_field(FieldQuantity q, int p, const double* d_x, double* d_out, hipStream_t s);
  // The flow execute (fmmbem_plan_execute_flow): velocity, pressure and velocity gradient on one far chain
  int flow_refusal(int p) const;
  int near_potential(bool near_f32, hipStream_t s);
  int deliver_field(FieldQuantity q, double* d_out, hipStream_t s) const;
  int run_flow(int p, const double* d_x, double* d_u, double* d_q, double* d_G, hipStream_t s);
  enum : int { kFlowNearNone = 0, kFlowNearFused = 2, kFlowNearSingle = 3 };       // fmmbem_stats.last_near_f32 after a flow execute
  // The representation execute (fmmbem_plan_execute_representation): both Laplace layers, value and gradient, on one far chain.
  // Its own buffers, allocated at first use: mu in tree order beside x_tree; the value's tree buffer -- hp.n doubles, the target
  // rows at n_src as l2p_kernel indexes y --, its distinct points and its staging (the gradient's are field[Gradient]'s); the
  // device copy of the one-slot view the far chain runs on (M2L above the rotation orders reads the plan from device memory)
  struct Representation {
    double *mu_tree = nullptr, *phi_tree = nullptr, *phi_points = nullptr, *phi_stage = nullptr, *stage_mu = nullptr;
    const DevicePlan* view_dev = nullptr;
  };
  Representation rep;
  size_t p2m_tab_doubles = 0;                                  // double2s of one P2M moment table (0: P2M runs without tables)
  int p2m_table(const uint8_t* bc, const double2** out);
  DevicePlan representation_view() const;
  int representation_refusal(int p) const;
  int representation_alloc(bool value, bool gradient);
  int run_representation(int p, const double* d_sigma, const double* d_mu, double* d_phi, double* d_grad, hipStream_t s);

  template <class V, class T>
  int upload(const V& v, const T** out) { return mem->upload(v, out); }
  template <class T>
  int alloc(size_t count, T** out, bool zero) { return mem->alloc(count, out, zero); }
  LayoutOptions layout_options() const;                      // the one place the layouts' options are filled in
  const double* create_vertices = nullptr;                   // fmmbem_plan_create: the caller's vertices while to_device_near runs (panel set-up on the device)
  // Geometry creation, the only writers of a PlanGeometry (-> shared).  to_device_near: the near field's share -- panels, leaves,
  // near lists, and the flag side's assembly LAUNCHED (to_device_bc_begin) -- as soon as the host plan holds them
  // (HostOptions::after_near_lists); to_device_far: the rest, when the host plan is complete, then to_device_bc_end
  int to_device_near(PlanGeometry& g);
  int to_device_far(PlanGeometry& g);
  int open_device();                                         // this plan's stream and event ring
  // what depends on the boundary-condition flags (-> this plan)
  void compose_d();
  int to_device_bc(const uint8_t* bc_tree);
  int to_device_bc_begin(const uint8_t* bc_tree);
  int to_device_bc_end();
  hipEvent_t asm_ev[2] = {nullptr, nullptr};                 // around the assembly, between to_device_bc_begin and _end
  static int like(std::shared_ptr<PlanShared> sh, const fmmbem_options& o, const uint8_t* bc, fmmbem_plan** out);
  int run(int p, const double* d_x, double* d_y, hipStream_t s, bool near_only, Phase phase = Phase::Whole, double* xbuf = nullptr);
  // Batched execute (fmmbem_plan_execute_batch).  Per vector of a pass: tree-order x and y, one multipole set, and a copy of d
  // pointing at them in device memory (the double-sum M2L reads the plan from there); allocated at the first batch call, kept
  // until destroy.  L, Mh and the target plans' y_points are shared: the vectors run the far field one after another.
  struct BatchBufs {
    int width = 0;                                             // 0: not allocated
    double* xt[kBatchMax] = {};
    double* yt[kBatchMax] = {};
    double2* M[kBatchMax] = {};
    DevicePlan* dev[kBatchMax] = {};
  };
  BatchBufs bat;
  DevicePlan batch_view(const BatchBufs& b, int j) const { DevicePlan dj = d; dj.xt = b.xt[j]; dj.yt = b.yt[j]; dj.M = b.M[j]; return dj; }   // d on vector j's buffers
  int batch_width() const;                                     // > 1: the fast path (one near-field pass for several vectors)
  int batch_alloc(hipStream_t s);
  int run_batch(int p, int k, const double* x, size_t ldx, double* y, size_t ldy, hipStream_t s, bool host);
  ~fmmbem_plan() {
    if (solver_ws) fmmbem::solver_ws_destroy(solver_ws);
    if (on_device) {
      DeviceGuard guard(opts.device);
      block_inverse_free();
      allocs.free_all();
      for (auto& e : ev) if (e) (void)hipEventDestroy(e);
      for (hipEvent_t e : asm_ev) if (e) (void)hipEventDestroy(e);      // a creation that failed between to_device_bc_begin and _end
      for (auto& ge : graphs) if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
      if (own_stream) (void)hipStreamDestroy(own_stream);
      if (hyb.recompute) (void)hipStreamDestroy(hyb.recompute);
      for (hipEvent_t e : {hyb.fork, hyb.join_recompute}) if (e) (void)hipEventDestroy(e);
    }
  }
};

// rot_tgt of a plan whose rotation pairs are its CSR lists: pair i belongs to the box b with m2l_ptr[b] <= i < m2l_ptr[b + 1]
__global__ void expand_csr_targets_kernel(const int* __restrict__ ptr, int nboxes, int* __restrict__ tgt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nboxes) return;
  for (int i = ptr[b]; i < ptr[b + 1]; ++i) tgt[i] = b;
}

// a target plan whose targets coincide: y[k] = y_points[point[k]] over the targets as given, dof unknowns per target (interleaved);
// n: unknowns, one thread each
__global__ void expand_targets_kernel(const uint32_t* __restrict__ point, const double* __restrict__ yp, double* __restrict__ y, int64_t n, int dof) {
  const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (u < n) {
    const int64_t k = u / dof;
    y[u] = yp[(int64_t)point[k] * dof + (u - k * dof)];
  }
}

// phase times of a plan build on stderr (FMMBEM_BUILD_TRACE: tuning aid)
struct BuildTrace {
  const bool on = sw::build_trace();
  double t_last = now_ms();
  void operator()(const char* what) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const double now = now_ms();
    std::fprintf(stderr, "to_device %-28s %8.2f ms\n", what, now - t_last);
    t_last = now;
  }
};

int fmmbem_plan::open_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMMBEM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU execution path)");
  if (opts.device < 0 || opts.device >= ndev) return fail(FMMBEM_ERR_INVALID, "device ordinal out of range");
  DEVICE_SCOPE(opts.device);
  on_device = true;
  allocs.device = opts.device;
  HIP_TRY(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
  ev.assign((size_t)kRing * 2 * kStages, nullptr);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  use_graphs = sw::graph(use_graphs);
  return FMMBEM_OK;
}

// what plan_layout.hpp takes from the options, the switches and the kernels' translation units
LayoutOptions fmmbem_plan::layout_options() const {
  LayoutOptions o;
  o.dof = opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1;
  o.sparse_local = opts.sparse_local != 0;
  o.treecode = treecode();
  o.targets = targets;
  o.near_stream_fraction = sw::near_stream_fraction(opts.near_stream_fraction);
  o.stokes_sym = sw::stokes_sym();
  o.m2l_rot = sw::m2l_rot();
  o.near_f32_max_p = opts.near_f32_max_p;
  o.rcg_item_rows = rcg_item_rows();
  o.l2p_group_leaves = l2p_group_leaves(opts.kernel);
  return o;
}

int fmmbem_plan::to_device_near(PlanGeometry& g) {
  TRY(open_device());
  DEVICE_SCOPE(opts.device);
  shared->allocs.device = opts.device;                 // a creation that fails from here on (an allocation, say the float near field's
  mem = &shared->allocs;                               // copy) frees the geometry's uploads with the plan: nothing stays behind
  BuildTrace mark;
  const HarmonicTables T;
  const int nl = hp.nleaves(), nb = hp.nboxes, pm = hp.opt.p_max;
  DevicePlan& d = g.gd;                                // the geometry's fields of the plan's d; compose_d adds the flag side
  mark("streams, events, tables");
  d = DevicePlan{};
  d.n = hp.n; d.nq = hp.rule.n; d.nboxes = nb; d.nleaves = nl;
  d.p_max = pm; d.s_max = pm * (pm + 1) / 2; d.p2_max = pm * pm; d.y2_max = 4 * pm * pm;
  // stride of a panel's P2M record: S(p_max) rounded up to 8 complex = 128 bytes, so that every record of the streamed table
  // starts on a cache line (55 -> 56 at p_max = 10: 0.244 -> 0.220 ms).  Not for M and L: the M2L kernel gathers them lane by
  // lane and is 9 % SLOWER with line-aligned boxes (0.56 -> 0.61 ms at p = 10)
  d.p2m_stride = (d.s_max + 7) & ~7;
  if ((d.p2m_stride - d.s_max) * 32 > d.s_max) d.p2m_stride = d.s_max;      // more than 3 % of padding (36 -> 40 at p_max = 8) costs more than it saves
  if (opts.kernel != FMMBEM_KERNEL_STOKES_BEM) {
    // Laplace: packed records (device_plan.hpp p2m_packed) -- the zero imaginary parts of the m = 0 moments are not stored
    d.p2m_packed = 1;
    d.p2m_real_off = pm * (pm - 1) / 2;
    const int len = d.p2m_real_off + (pm + 1) / 2;                          // the reals two to a double2 slot
    d.p2m_stride = (len + 7) & ~7;
    if ((d.p2m_stride - len) * 32 > len) d.p2m_stride = len;                // the same 3 % rule: 50 slots = 800 bytes at p_max = 10, 72 = 1 152 at 12
  }
  d.leaf_begin = hp.leaf_begin; d.leaf_end = hp.leaf_end; d.row_begin = hp.row_begin; d.row_end = hp.row_end;
  for (int q = 0; q < hp.rule.n; ++q) d.qw[q] = hp.rule.w[q];
  d.kernel = opts.kernel;
  if (opts.kernel == FMMBEM_KERNEL_STOKES_BEM) {
    d.dof = 3; d.mu = opts.mu;
    QuadRule fine;
    if (!quad_rule(opts.quad_k_fine, fine)) return fail(FMMBEM_ERR_INVALID, "invalid K_fine (valid: 1 3 4 7 13 17 19 25 79)");
    d.nqf = fine.n;
    std::vector<double> qf((size_t)fine.n * 4);
    for (int q = 0; q < fine.n; ++q) { for (int k = 0; k < 3; ++k) qf[4 * q + k] = fine.pts[q][k]; qf[4 * q + 3] = fine.w[q]; }
    TRY(upload(qf, &d.qf));
  } else {
    d.dof = 1;
  }
  const int dof = d.dof;

  // panels + permutation
  TRY(upload(hp.perm, &d.perm));
  if (create_vertices) {
    // the panels' derived geometry, computed on the device from the caller's vertices (kernels_near.hip panel_setup: the host
    // form's arithmetic, bit for bit): 75 MB up instead of 0.2 GB written by the host and then uploaded
    const size_t nn = (size_t)hp.n;
    double *cx, *cy, *cz, *nx, *ny, *nz, *ar, *qd, *vt;
    TRY(alloc(nn, &cx, false)); TRY(alloc(nn, &cy, false)); TRY(alloc(nn, &cz, false));
    TRY(alloc(nn, &nx, false)); TRY(alloc(nn, &ny, false)); TRY(alloc(nn, &nz, false));
    TRY(alloc(nn, &ar, false)); TRY(alloc(nn * 3 * hp.rule.n, &qd, false)); TRY(alloc(nn * 9, &vt, false));
    double* v_orig = nullptr;
    HIP_TRY(hipMalloc(&v_orig, sizeof(double) * 9 * nn));
    std::vector<double> pts((size_t)hp.rule.n * 3);
    for (int q = 0; q < hp.rule.n; ++q) for (int k = 0; k < 3; ++k) pts[3 * q + k] = hp.rule.pts[q][k];
    const double* d_pts = nullptr;
    hipError_t e = hipMemcpy(v_orig, create_vertices, sizeof(double) * 9 * nn, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? upload(pts, &d_pts) : FMMBEM_ERR_HIP;
    if (rc == FMMBEM_OK) e = launch_panel_setup(hp.n, d.perm, v_orig, hp.rule.n, d_pts, cx, cy, cz, nx, ny, nz, ar, qd, vt, own_stream);
    if (rc == FMMBEM_OK && e == hipSuccess) e = hipStreamSynchronize(own_stream);
    (void)hipFree(v_orig);
    if (rc != FMMBEM_OK) return rc;
    if (e != hipSuccess) return fail(FMMBEM_ERR_HIP, std::string("panel setup: ") + hipGetErrorString(e));
    d.cx = cx; d.cy = cy; d.cz = cz; d.nx = nx; d.ny = ny; d.nz = nz; d.area = ar; d.quad = qd; d.vert = vt;
  } else {
    const PanelSoA& P = hp.panels;
    TRY(upload(P.cx, &d.cx)); TRY(upload(P.cy, &d.cy)); TRY(upload(P.cz, &d.cz));
    TRY(upload(P.nx, &d.nx)); TRY(upload(P.ny, &d.ny)); TRY(upload(P.nz, &d.nz));
    TRY(upload(P.area, &d.area)); TRY(upload(P.quad, &d.quad)); TRY(upload(P.vert, &d.vert));
  }

  mark("panels: upload + geometry");
  // leaves, the near block structure, the work items of every near-field form: decided in plan_layout.hpp, uploaded here
  NearLayout L = near_layout(hp, layout_options());
  g.hybrid = L.hybrid; g.near_recomputed_pairs = L.near_recomputed_pairs;
  d.max_runs = L.max_runs; d.max_ncols = L.max_cols;
  if (!layout_options().m2l_rot) g.rot_max = 0;
  g.near_total_doubles = L.near_total_doubles; g.sym_total_doubles = L.sym_total_doubles;      // allocated per plan (to_device_bc_begin)
  g.near_f32_floats = L.near_f32_floats; g.near_bytes = L.near_bytes;
  TRY(upload(L.leaf_row0, &d.leaf_row0)); TRY(upload(L.leaf_nrows, &d.leaf_nrows)); TRY(upload(hp.leaf_box, &d.leaf_box));
  TRY(upload(L.run_ptr, &d.near_ptr)); TRY(upload(L.run_row0, &d.near_run_row0)); TRY(upload(L.run_off, &d.near_run_off));
  TRY(upload(hp.near_ncols, &d.near_ncols)); TRY(upload(L.near_stride, &d.near_stride)); TRY(upload(L.near_off, &d.near_off));
  d.near_nitems = (int)L.items.size();
  TRY(upload(L.items, &d.near_items)); TRY(upload(L.recs, &d.near_recs));
  if (L.stokes_sym) {
    d.sym_nitems = (int)L.sym_items.size();
    TRY(upload(L.sym_items, &d.sym_items)); TRY(upload(L.sym_off, &d.near_sym_off));
  }
  if (L.f32) {
    TRY(upload(L.off32, &d.near_f32_off));
    if (dof == 1) TRY(upload(L.recs32, &d.near_recs_f32));
  }
  if (L.hybrid) {
    // the side listing (mf_sweep COUNT / FILL) walks d.near_items: the recompute items, panel rows
    d.near_nitems_stream = dof == 1 ? d.near_nitems : 0;   // (Laplace: the items uploaded above are the streamed ones, near_recs)
    d.near_nitems = (int)L.rc_items.size();
    TRY(upload(L.rc_items, &d.near_items));
    d.rc_nitems = (int)L.rc_recs.size();
    TRY(upload(L.rc_recs, &d.rc_items));
    TRY(upload(L.rec, &d.near_rec));
    if (dof == 3) {
      // packed per-panel records of near_recompute3g_kernel (its sources go straight into LDS, 16 bytes at a time)
      double *rs = nullptr, *rn = nullptr;
      TRY(alloc((size_t)hp.n * 16, &rs, false)); TRY(alloc((size_t)hp.n * 4, &rn, false));
      HIP_TRY(launch_rc_pack(d, rs, rn, own_stream));
      HIP_TRY(hipStreamSynchronize(own_stream));
      d.rc_src = rs; d.rc_nrm = rn;
    }
  }
  g.near_rec_host = std::move(L.rec); g.near_off_host = std::move(L.near_off); g.sym_off_host = std::move(L.sym_off);      // (introspection)

  mark("near lists + items");
  // boxes, expansions, tables
  TRY(upload(hp.box_center, &d.box_center));
  TRY(upload(T.A, &d.tabA)); TRY(upload(T.invA, &d.tabInvA)); TRY(upload(T.pref, &d.tabPref));
  TRY(upload(step_table(T), &d.tabStep));

  mark("boxes + harmonic tables");
  return to_device_bc_begin(hp.panels.bc.data());    // the near-matrix assembly runs on the GPU from here, under the host work that follows
}

int fmmbem_plan::to_device_far(PlanGeometry& g) {
  DEVICE_SCOPE(opts.device);
  mem = &shared->allocs;
  BuildTrace mark;
  const HarmonicTables T;
  const int nb = hp.nboxes, pm = hp.opt.p_max;
  DevicePlan& d = g.gd;
  // every list, record and class table of the far field: decided in plan_layout.hpp, uploaded here
  FarLayout F = far_layout(hp, T, layout_options());
  d.n_p2m = (int)F.p2m_leaf.size(); d.n_l2p = (int)F.l2p_leaf.size();
  TRY(upload(F.p2m_leaf, &d.p2m_leaf)); TRY(upload(F.l2p_leaf, &d.l2p_leaf));
  d.n_l2p_grp = F.n_l2p_grp;
  TRY(upload(F.l2p_grp, &d.l2p_grp));
  g.l2p_scatter = F.l2p_scatter;
  TRY(upload(hp.m2m_parents, &d.m2m_parent)); TRY(upload(hp.l2l_children, &d.l2l_child));
  TRY(upload(hp.box_child_begin, &d.box_child_begin)); TRY(upload(hp.box_child_end, &d.box_child_end));
  TRY(upload(hp.box_parent, &d.box_parent));
  g.up.launch = std::move(F.up.launch); g.down.launch = std::move(F.down.launch); g.m2m_shared_launch = std::move(F.shared_launch);
  g.up.rot = std::move(F.up.rot); g.down.rot = std::move(F.down.rot); g.m2m_shared_rot = std::move(F.shared_rot);
  // sharded upward pass: who sends which multipoles
  g.split_upward = hp.opt.shard_upward && hp.opt.shard_world > 1;
  d.xch_rank = hp.opt.shard_rank; d.xch_world = g.split_upward ? hp.opt.shard_world : 0; d.xch_max = 0;
  for (int r = 0; r < 9; ++r) d.xch_ptr[r] = 0;
  if (g.split_upward) {
    if (hp.opt.shard_world > 8) return fail(FMMBEM_ERR_UNSUPPORTED, "sharded upward pass: at most 8 shards");
    for (int r = 0; r <= hp.opt.shard_world; ++r) d.xch_ptr[r] = hp.xch_ptr[r];
    for (int r = 0; r < hp.opt.shard_world; ++r) d.xch_max = std::max(d.xch_max, hp.xch_ptr[r + 1] - hp.xch_ptr[r]);
  }
  TRY(upload(hp.xch_box, &d.xch_box));
  if (g.split_upward && hp.opt.shard_upward == 2) {      // selective exchange: only what the receiver reads
    TRY(upload(hp.xsel_send_box, &d.xsel_send_box)); TRY(upload(hp.xsel_recv_box, &d.xsel_recv_box));
    d.xsel_send_n = (int)hp.xsel_send_box.size(); d.xsel_recv_n = (int)hp.xsel_recv_box.size();
  }

  mark("far-field lists");
  const std::shared_ptr<const OrderTables> otp = order_tables().get();      // (built on a thread of their own since plan_create began)
  const OrderTables& ot = *otp;
  // parent<->child translation classes; M2M / L2L by rotation: pair lists per level launch, items, records, constant streams
  TRY(upload(F.up_cls, &d.up_cls)); TRY(upload(F.down_cls, &d.down_cls));
  TRY(upload(F.up.rec, &g.up.rec)); TRY(upload(F.down.rec, &g.down.rec));
  auto upload_pairs = [&](const SideLayout& from, ShiftSide& sd) -> int {
    TRY(upload(from.src, &sd.rsrc)); TRY(upload(from.cls, &sd.rcls)); TRY(upload(from.tgt, &sd.rtgt)); TRY(upload(from.item, &sd.ritem));
    return FMMBEM_OK;
  };
  TRY(upload_pairs(F.up, g.up)); TRY(upload(F.up_unit_ptr, &g.up.unit_ptr));
  TRY(upload_pairs(F.down, g.down));
  std::copy(ot.shift_off, ot.shift_off + kRotPmax, g.shift_stream_off);
  TRY(upload(ot.ups, &g.up.stream)); TRY(upload(ot.dns, &g.down.stream));
  // one pair per wavefront: class tables and the lanes' tables per order
  TRY(upload(F.up.sl_class, &g.up.sl_class)); TRY(upload(F.down.sl_class, &g.down.sl_class));
  std::copy(ot.sl_rot_off, ot.sl_rot_off + kShiftLanesPmax + 1, g.sl_rot_off);
  std::copy(ot.sl_ax_off, ot.sl_ax_off + kShiftLanesPmax + 1, g.sl_ax_off);
  TRY(upload(ot.urc, &g.up.sl_rc)); TRY(upload(ot.urs, &g.up.sl_rs)); TRY(upload(ot.uxc, &g.up.sl_xc)); TRY(upload(ot.uxs, &g.up.sl_xs));
  TRY(upload(ot.drc, &g.down.sl_rc)); TRY(upload(ot.drs, &g.down.sl_rs)); TRY(upload(ot.dxc, &g.down.sl_xc)); TRY(upload(ot.dxs, &g.down.sl_xs));
  g.shift_lanes = sw::shift_lanes(g.shift_lanes);
  g.shift_lanes_max = sw::shift_lanes_max(g.shift_lanes_max);
  g.shift_rot = sw::shift_rot(g.shift_rot);
  g.shift_rot_min = sw::shift_rot_min(g.shift_rot_min);
  {
    const cplx *pu = nullptr, *pd = nullptr;
    TRY(upload(F.up_tab, &pu)); TRY(upload(F.down_tab, &pd));
    d.up_tab = reinterpret_cast<const double2*>(pu);
    d.down_tab = reinterpret_cast<const double2*>(pd);
  }
  TRY(upload_shift_ops(*mem, build_shift_ops(pm, T.A, kEps), g.up.ops, g.down.ops));

  mark("shift classes + operators");
  // M2L: targets to run, sources whose Mh is needed, class tables Yh[r,c] = i^{|c|} EPS Y[r,c] / A[r,c]
  d.n_m2l_tgt = (int)F.m2l_tgt.size(); d.n_mh = (int)F.mh_box.size();
  TRY(upload(F.m2l_tgt, &d.m2l_tgt)); TRY(upload(F.mh_box, &d.mh_box));
  TRY(upload(hp.m2l_ptr, &d.m2l_ptr)); TRY(upload(hp.m2l_src, &d.m2l_src)); TRY(upload(hp.m2l_cls, &d.m2l_cls));
  if (treecode()) {                                    // M2P work (device_launch.hpp M2PWork)
    g.m2p.n_items = (int)F.m2p_item_leaf.size();
    TRY(upload(F.m2p_item_leaf, &g.m2p.item_leaf)); TRY(upload(F.m2p_item_row, &g.m2p.item_row));
    TRY(upload(F.m2p_chain_ptr, &g.m2p.chain_ptr)); TRY(upload(F.m2p_chain_box, &g.m2p.chain_box));
  }
  mark("m2l lists upload");
  g.n_classes = F.n_classes;
  d.g_max = F.g_max;
  {
    const cplx* pz = nullptr;
    TRY(upload(F.m2l_g, &d.m2l_g));
    TRY(upload(F.m2l_z, &pz));
    d.m2l_z = reinterpret_cast<const double2*>(pz);
  }
  // lane -> output maps and table -> LDS scatter maps of the M2L kernel, every order up to p_max
  if (!ot.lanes_ok) return fail(FMMBEM_ERR_INVALID, "internal: M2L lane dealing failed");
  std::copy(ot.scat_off, ot.scat_off + kPmax, d.m2l_scat_off);
  TRY(upload(ot.lanes, &d.m2l_lane)); TRY(upload(ot.scat, &d.m2l_scat));

  mark("m2l class tables");
  // M2L by rotation (kernels_m2l_rot.hip): the owned pairs in CSR order by target, cut into items; class records; constants
  d.n_rot_items = (int)hp.rot_item_ptr.size() - 1;
  d.n_rot_empty = (int)hp.rot_empty.size();
  if (hp.rot_alias) {
    // one pair list for both M2L kernels; the target of pair i is the box whose CSR range holds i (written on the device)
    d.rot_src = d.m2l_src; d.rot_cls = d.m2l_cls;
    int* tgt = nullptr;
    TRY(alloc(hp.m2l_src.size(), &tgt, false));
    if (nb > 0) hipLaunchKernelGGL(expand_csr_targets_kernel, dim3((nb + 255) / 256), dim3(256), 0, own_stream, d.m2l_ptr, nb, tgt);
    HIP_TRY(hipGetLastError());
    d.rot_tgt = tgt;
  } else {
    TRY(upload(hp.rot_src, &d.rot_src)); TRY(upload(hp.rot_cls, &d.rot_cls)); TRY(upload(hp.rot_tgt, &d.rot_tgt));
  }
  TRY(upload(hp.rot_item_ptr, &d.rot_item_ptr)); TRY(upload(hp.rot_empty, &d.rot_empty));
  d.n_rot_items_long = (int)hp.rot_item_ptr_long.size() - 1;
  TRY(upload(hp.rot_item_ptr_long, &d.rot_item_ptr_long));
  TRY(upload(F.rot_cls_rec, &d.rot_cls_rec));
  std::copy(ot.rot_off, ot.rot_off + kRotPmax, d.rot_tab_off);
  TRY(upload(ot.rot_all, &d.rot_tab));

  mark("rotation lists");
  return to_device_bc_end();
}

// Everything of a plan that depends on the boundary-condition flags: which expansion slots are live, the flags themselves, the
// near-matrix values (the TARGET's flag picks the kernel), the P2M moments (the SOURCE's flag picks them), the expansions and the
// work vectors.  bc_tree: the flags in tree order.  Allocations go to this plan, not to the shared block.
int fmmbem_plan::to_device_bc(const uint8_t* bc_tree) {
  TRY(to_device_bc_begin(bc_tree));
  return to_device_bc_end();
}

// The one place a plan's d is made, fresh plan or derived: the geometry's fields as they stand, then every field of the flag side
// (a field that is not listed here is null in every plan)
void fmmbem_plan::compose_d() {
  d = g.gd;
  d.bc = fd.bc; d.n_act = fd.n_act; d.nslots = fd.nslots;
  for (int i = 0; i < 12; ++i) d.act[i] = fd.act[i];
  d.stokes_velocity_targets = fd.stokes_velocity_targets; d.stokes_traction_targets = fd.stokes_traction_targets;
  d.near_val = fd.near_val; d.near_sym = fd.near_sym; d.near_f32 = fd.near_f32;
  d.ys = fd.ys; d.xt4 = fd.xt4;
  d.M = fd.M; d.L = fd.L; d.Mh = fd.Mh; d.xt = fd.xt; d.yt = fd.yt;
  d.p2m_tab = fd.p2m_tab; d.p2m_tab_g = fd.p2m_tab_g; d.p2m_tab_row0 = fd.p2m_tab_row0;
  d.side_ptr = fd.side_ptr; d.side_col = fd.side_col; d.side_val = fd.side_val; d.side_items = fd.side_items; d.side_nitems = fd.side_nitems;
}

// First half: the flags, the near-matrix storage, and the assembly LAUNCHED (own_stream, asynchronous) -- to_device_near calls this as
// soon as the panels and the near lists are in HBM, so that the 20-50 ms of panel integrals run on the GPU while the host goes on
// tabulating and uploading the far-field operators.
int fmmbem_plan::to_device_bc_begin(const uint8_t* bc_tree) {
  DEVICE_SCOPE(opts.device);
  mem = &allocs;
  fd.n_act = 0;
  if (opts.kernel == FMMBEM_KERNEL_STOKES_BEM) {
    // StokesSphericalBEM: M[2][4] per box (kernel/StokesSphericalBEM.hpp:143-153).  The TARGET's flag picks the operator
    // (:377-389): velocity targets read the four potentials of the single layer (slots 0..3), TRACTION targets the seven of
    // the double layer (slots 4..10, kernels_far.hip p2m_apply_kernel<3>); every source feeds the groups that have readers
    fd.stokes_velocity_targets = has_bc[0] ? 1 : 0;
    fd.stokes_traction_targets = (has_bc[1] && hp.opt.evaluator == 0) ? 1 : 0;
    if (!fd.stokes_velocity_targets && !fd.stokes_traction_targets) fd.stokes_velocity_targets = 1;
    fd.nslots = fd.stokes_traction_targets ? 11 : 8;
    if (fd.stokes_velocity_targets) for (int s = 0; s < 4; ++s) fd.act[fd.n_act++] = s;
    if (fd.stokes_traction_targets) for (int s = 4; s < 11; ++s) fd.act[fd.n_act++] = s;
  } else {
    fd.nslots = 2;
    for (int s = 0; s < 2; ++s) if (has_bc[s]) fd.act[fd.n_act++] = s;
  }
  {
    uint8_t* dbc = nullptr;
    TRY(alloc((size_t)hp.n, &dbc, false));
    HIP_TRY(hipMemcpy(dbc, bc_tree, (size_t)hp.n, hipMemcpyHostToDevice));
    fd.bc = dbc;
  }
  for (int f = 0; p2m_per_slot() && f < 2; ++f) {
    uint8_t* all = nullptr;
    TRY(alloc((size_t)hp.n, &all, false));
    HIP_TRY(hipMemset(all, f, (size_t)hp.n));
    bc_all[f] = all;
  }
  if (g.near_total_doubles) TRY(alloc((size_t)g.near_total_doubles, &fd.near_val, false));
  if (g.sym_total_doubles) TRY(alloc((size_t)g.sym_total_doubles, &fd.near_sym, false));
  if (g.near_f32_floats) TRY(alloc((size_t)g.near_f32_floats, &fd.near_f32, false));
  if (g.hybrid) {
    HIP_TRY(hipStreamCreateWithFlags(&hyb.recompute, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&hyb.fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&hyb.join_recompute, hipEventDisableTiming));
    TRY(alloc((size_t)hp.n * g.gd.dof, &fd.ys, true));
    if (g.gd.rc_src) TRY(alloc((size_t)hp.n * 4, &fd.xt4, true));
  }
  compose_d();
  // near-field assembly on the device, in flight from here on (everything it reads is uploaded; to_device_bc_end waits for it)
  HIP_TRY(hipEventCreate(&asm_ev[0])); HIP_TRY(hipEventCreate(&asm_ev[1]));
  HIP_TRY(hipEventRecord(asm_ev[0], own_stream));
  if (opts.sparse_local) {
    if (opts.kernel == FMMBEM_KERNEL_STOKES_BEM) HIP_TRY(launch_near_assemble_stokes(d, own_stream));
    else HIP_TRY(launch_near_assemble(d, own_stream));
    if (fd.near_f32) HIP_TRY(launch_near_to_f32(d, own_stream));      // the float copy of what was just assembled
  }
  HIP_TRY(hipEventRecord(asm_ev[1], own_stream));
  return FMMBEM_OK;
}

int fmmbem_plan::to_device_bc_end() {
  DEVICE_SCOPE(opts.device);
  mem = &allocs;
  BuildTrace mark;
  const int dof = g.gd.dof, nb = hp.nboxes;
  TRY(alloc((size_t)nb * fd.nslots * g.gd.s_max, &fd.M, true));
  TRY(alloc((size_t)nb * fd.nslots * g.gd.s_max, &fd.L, true));
  TRY(alloc((size_t)nb * fd.nslots * g.gd.s_max, &fd.Mh, true));
  TRY(alloc((size_t)hp.n * dof, &fd.xt, true));
  TRY(alloc((size_t)hp.n * dof, &fd.yt, true));
  TRY(alloc((size_t)hp.n * dof, &stage_x, true));
  TRY(alloc((size_t)hp.n * dof, &stage_y, true));

  // The zero-fills above ran on the NULL stream, which the plan's non-blocking streams do not wait for:
  // drain it before anything else touches those buffers (a late memset of x_tree / staging vectors would
  // otherwise race with the first execute).
  HIP_TRY(hipDeviceSynchronize());

  mark("vectors");
  // P2M as a stored operator: every panel's moments about its leaf centre, at p_max (FMMBEM_P2M_TABLE=0, or more than
  // 16 GB of them: the recurrences are run every matvec instead)
  {
    const bool table_on = sw::p2m_table();
    const size_t ntab = opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 4 : 1;
    // the panels of the leaves this plan runs P2M on: all of them, or -- upward pass sharded by owner -- the shard's own
    // rows only (0.9 GB at N = 1M, p_max = 10 for the whole mesh: one eighth of that per GPU on an 8-GPU node)
    int64_t r0 = hp.n, r1 = 0;
    for (int b : hp.p2m_leaves) { r0 = std::min<int64_t>(r0, hp.box_body_begin[b]); r1 = std::max<int64_t>(r1, hp.box_body_end[b]); }
    if (r1 < r0) r0 = r1 = 0;
    fd.p2m_tab_row0 = r0;
    compose_d();                                       // the geometry is complete by now: the tables are built from the whole of d
    const size_t count = (size_t)(r1 - r0) * ntab * d.p2m_stride;
    const bool stokes = opts.kernel == FMMBEM_KERNEL_STOKES_BEM;
    const size_t count_g = (size_t)(r1 - r0) * 3 * d.p2m_stride;
    if (stokes && fd.stokes_traction_targets && d.n_p2m > 0 && table_on && count_g * sizeof(double2) <= ((size_t)16 << 30)) {
      // the double layer's gradient records; without them (switch, or more than 16 GB) its P2M runs the recurrences per matvec
      double2* tab = nullptr;
      TRY(alloc(count_g, &tab, true));
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(launch_p2m_table_grad(d, tab, own_stream));
      HIP_TRY(hipStreamSynchronize(own_stream));
      fd.p2m_tab_g = tab;
    }
    const bool want = !stokes || fd.stokes_velocity_targets;
    if (want && table_on && hp.opt.evaluator == 0 && d.n_p2m > 0 && count * sizeof(double2) <= ((size_t)16 << 30)) {
      const bool per_slot = p2m_per_slot();
      p2m_tab_doubles = count;
      for (int f = 0; f < 2; ++f) {                    // (a Laplace dual plan: the table of every live slot, all sources; else one table)
        if (per_slot && !has_bc[f]) continue;
        TRY(p2m_table(per_slot ? bc_all[f] : d.bc, &p2m_tab_slot[f]));
        if (!per_slot) break;
      }
      fd.p2m_tab = p2m_tab_slot[0] ? p2m_tab_slot[0] : p2m_tab_slot[1];
    }
  }
  compose_d();
  mark("p2m table");
  // the near-field assembly launched by to_device_bc_begin: its device time
  HIP_TRY(hipStreamSynchronize(own_stream));
  {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, asm_ev[0], asm_ev[1]));
    build_assemble_ms = ms;
    (void)hipEventDestroy(asm_ev[0]); (void)hipEventDestroy(asm_ev[1]);
    asm_ev[0] = asm_ev[1] = nullptr;
  }
  const double t0 = now_ms();
  if ((!opts.sparse_local || g.hybrid) && hp.row_end > hp.row_begin) TRY(build_side_lists());
  build_assemble_ms += now_ms() - t0;
  mark("near assembly (waited for)");
  compose_d();
  {                                                    // the plan itself, readable from the device
    TRY(allocs.upload(&d, 1, &d_dev));
  }
  return FMMBEM_OK;
}

// matrix-free plans (every owned row) and hybrid plans (the rows of the recomputed leaves; the others list nothing):
int fmmbem_plan::build_side_lists() {
  const int dof = d.dof;
  {
    // nothing is assembled for these rows, but the pairs of the near regimes -- the expensive 4.5 %, the same numbers every matvec
    // -- are listed per target row and evaluated once (kernels_near.hip, near_matfree third form): count, scan, fill, evaluate
    int* d_cnt = nullptr;
    TRY(alloc((size_t)hp.n, &d_cnt, true));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(launch_mf_side(d, 0, d_cnt, nullptr, nullptr, nullptr, nullptr, 0, own_stream));
    HIP_TRY(hipStreamSynchronize(own_stream));
    std::vector<int> cnt((size_t)hp.n);
    HIP_TRY(hipMemcpy(cnt.data(), d_cnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    std::vector<int64_t> ptr((size_t)hp.n + 1, 0);
    for (int64_t i = 0; i < hp.n; ++i) ptr[(size_t)i + 1] = ptr[(size_t)i] + cnt[(size_t)i];
    const int64_t nside = ptr.back();
    std::vector<int> row((size_t)nside);
    for (int64_t i = 0; i < hp.n; ++i)
      for (int64_t k = ptr[(size_t)i]; k < ptr[(size_t)i + 1]; ++k) row[(size_t)k] = (int)i;
    const int* d_row = nullptr;
    int* d_col = nullptr;
    double* d_val = nullptr;
    TRY(upload(ptr, &fd.side_ptr)); TRY(upload(row, &d_row));
    TRY(alloc((size_t)nside, &d_col, false)); TRY(alloc((size_t)nside * (dof == 3 ? 9 : 1), &d_val, false));
    HIP_TRY(launch_mf_side(d, 1, nullptr, fd.side_ptr, d_col, nullptr, nullptr, nside, own_stream));
    HIP_TRY(launch_mf_side(d, 2, nullptr, nullptr, d_col, d_row, d_val, nside, own_stream));
    HIP_TRY(hipStreamSynchronize(own_stream));
    fd.side_col = d_col; fd.side_val = d_val;
    near_side_entries = nside;
    if (g.hybrid) {                                    // work items of near_side_items (kernels_near.hip)
      const std::vector<int4> sitems = cut_side_items(cnt, ptr, hp.row_begin, hp.row_end);
      fd.side_nitems = (int)sitems.size();
      TRY(upload(sitems, &fd.side_items));
    }
    allocs.free_one(d_cnt); allocs.free_one(d_row);          // creation-time scratch
  }
  return FMMBEM_OK;
}

// The upward / downward pass, level launch by level launch; each takes the kernel shift_form (launch_choice.hpp) names
int fmmbem_plan::shift_pass(const DevicePlan& dv, int p, ShiftDir dir, hipStream_t s) const {
  const bool m2m = dir != ShiftDir::Down;
  const ShiftSide& sd = m2m ? g.up : g.down;
  const auto& launches = dir == ShiftDir::UpShared ? g.m2m_shared_launch : sd.launch;
  const auto& rots = dir == ShiftDir::UpShared ? g.m2m_shared_rot : sd.rot;
  for (size_t i = 0; i < launches.size(); ++i) {
    const auto [first, count] = launches[i];
    const ShiftRot& sr = rots[i];
    const ShiftForm f = shift_form(g.shift_rot, g.shift_lanes, g.shift_lanes_max, g.shift_rot_min, sr.pairs, sr.level_boxes, p, dv.n_act, m2m,
                                   shift_lanes_supported(p), shift_rot_supported(p));
    if (f == ShiftForm::Lanes) {
      ShiftLaneWork lw;
      const int at = m2m ? 0 : sr.pair_first;          // L2L shifts its pair arrays to the launch's first pair (unit u is pair u); M2M takes them unshifted
      lw.src = sd.rsrc + at; lw.cls = sd.rcls + at; lw.tgt = sd.rtgt + at; lw.n_units = sr.n_units;
      lw.unit_ptr = m2m ? sd.unit_ptr + sr.unit_first : nullptr;   // M2M walks a parent's pairs through its unit pointer (positions in the unshifted arrays); L2L has none
      lw.class_tab = sd.sl_class; lw.class_stride = sl_class_doubles(hp.opt.p_max); lw.p_max = hp.opt.p_max;
      lw.rot_c = sd.sl_rc + g.sl_rot_off[p]; lw.rot_s = sd.sl_rs + g.sl_rot_off[p]; lw.ax_c = sd.sl_xc + g.sl_ax_off[p]; lw.ax_s = sd.sl_xs + g.sl_ax_off[p];
      HIP_TRY(m2m ? launch_m2m_lanes(dv, lw, p, s) : launch_l2l_lanes(dv, lw, p, s));
    } else if (f == ShiftForm::Rot) {
      RotWork w;
      w.src = sd.rsrc; w.cls = sd.rcls; w.tgt = sd.rtgt; w.rec = sd.rec;
      w.item_ptr = sd.ritem + sr.item_first; w.n_items = sr.n_items;
      w.stream = sd.stream + g.shift_stream_off[p - 1];
      HIP_TRY(m2m ? launch_m2m_rot(dv, w, p, s) : launch_l2l_rot(dv, w, p, s));
    } else HIP_TRY(m2m ? launch_m2m_level(dv, sd.ops[p - 1], p, first, count, s) : launch_l2l_level(dv, sd.ops[p - 1], p, first, count, s));
  }
  return FMMBEM_OK;
}

// One P2M moment table of p2m_tab_doubles records (kernels_far.hip, launch_p2m_table) with the panels' flags read from bc: the
// plan's own tables at creation, and the table of a slot the plan's targets do not make live at the first representation execute
int fmmbem_plan::p2m_table(const uint8_t* bc, const double2** out) {
  DevicePlan dt = d;
  dt.bc = bc;
  double2* tab = nullptr;
  TRY(alloc(p2m_tab_doubles, &tab, true));
  HIP_TRY(hipDeviceSynchronize());                     // the zero-fill ran on the NULL stream
  HIP_TRY(launch_p2m_table(dt, tab, own_stream));
  HIP_TRY(hipStreamSynchronize(own_stream));
  *out = tab;
  return FMMBEM_OK;
}

// P2M of a Laplace dual plan: once per live slot, every source panel taken with that slot's flag (the moments of G, or of dG/dn with the
// panel's normal) and that slot's table; the same kernels as a plan whose panels all carry the flag
template <class Launch>
int fmmbem_plan::p2m_targets(const DevicePlan& dv, Launch&& launch) const {
  for (int f = 0; f < 2; ++f) {
    if (!has_bc[f]) continue;
    DevicePlan dp = dv;
    dp.bc = bc_all[f];
    dp.n_act = 1; dp.act[0] = f;
    if (dv.p2m_tab) dp.p2m_tab = p2m_tab_slot[f];
    HIP_TRY(launch(dp));
  }
  return FMMBEM_OK;
}
// P2M on the view given: a Stokes plan's (a field plan too: every source feeds every live group), a Laplace dual plan's slot by
// slot, or the one launch
int fmmbem_plan::p2m(const DevicePlan& dv, int p, StageMarks& tm, hipStream_t s) const {
  auto one = [&](const DevicePlan& dp) { return launch_p2m(dp, p, s); };
  HIP_TRY(tm.begin(Stage::P2M, s));
  if (dv.kernel == FMMBEM_KERNEL_STOKES_BEM) HIP_TRY(launch_p2m_stokes(dv, p, s));
  else if (targets) TRY(p2m_targets(dv, one));
  else HIP_TRY(one(dv));
  HIP_TRY(tm.end(Stage::P2M, s));
  return FMMBEM_OK;
}
// L2P on the view given: y_tree += the far field; with y_out (Laplace, l2p_delivers) y_out[perm[i]] = y_tree[i] + the far field
int fmmbem_plan::l2p(const DevicePlan& dv, int p, double* y_out, hipStream_t s) const {
  if (dv.kernel == FMMBEM_KERNEL_STOKES_BEM) HIP_TRY(launch_l2p_stokes(dv, p, dv.yt, s));
  else HIP_TRY(launch_l2p(dv, p, dv.yt, s, y_out ? dv.perm : nullptr, y_out));
  return FMMBEM_OK;
}

// The far field after P2M on the view given -- the plan's d and its device copy; a batch: vector j's -- for every caller: the same
// launches in the same order, so the same bits.  m2m_own: M2M of the own boxes runs (not on the downward half of a split execute:
// the upward half ran it); xch: the other shards' multipoles are unpacked from it, then the parents spanning shards (null: neither)
int fmmbem_plan::far_chain(const DevicePlan& dv, const DevicePlan* dv_dev, int p, bool m2m_own, const double* xch, L2PTo to, double* y_out,
                           StageMarks& tm, hipStream_t s) const {
  if (m2m_own) {
    HIP_TRY(tm.begin(Stage::M2M, s));
    TRY(shift_pass(dv, p, ShiftDir::Up, s));
    HIP_TRY(tm.end(Stage::M2M, s));
  }
  if (treecode()) {                                    // (never a shard) the far field as one stage, timed as M2L's
    HIP_TRY(tm.begin(Stage::M2L, s));
    HIP_TRY(launch_m2p(dv, g.m2p, p, dv.yt, s));
    HIP_TRY(tm.end(Stage::M2L, s));
    return FMMBEM_OK;
  }
  HIP_TRY(tm.begin(Stage::Mh, s));
  if (xch) {
    HIP_TRY(launch_xch_unpack(dv, p, reinterpret_cast<const double2*>(xch), s));
    TRY(shift_pass(dv, p, ShiftDir::UpShared, s));
  }
  const bool rot = g.use_rot(p);
  if (!rot) HIP_TRY(launch_mh_prep(dv, p, s));       // the rotation kernel reads M itself
  HIP_TRY(tm.end(Stage::Mh, s));
  HIP_TRY(tm.begin(Stage::M2L, s));
  HIP_TRY(rot ? launch_m2l_rot(dv, dv_dev, p, s) : launch_m2l(dv, dv_dev, p, s));
  HIP_TRY(tm.end(Stage::M2L, s));
  HIP_TRY(tm.begin(Stage::L2L, s));
  TRY(shift_pass(dv, p, ShiftDir::Down, s));
  HIP_TRY(tm.end(Stage::L2L, s));
  HIP_TRY(tm.begin(Stage::L2P, s));
  if (to != L2PTo::Caller) TRY(l2p(dv, p, to == L2PTo::Perm ? y_out : nullptr, s));
  HIP_TRY(tm.end(Stage::L2P, s));
  return FMMBEM_OK;
}

// The result leaves the plan once, at the very end: the owned rows of y_tree (near + far field) scattered to the caller's
// panel order (zeros elsewhere when the plan is a shard), or -- result_slices -- copied as they are, tree order, to the
// head of d_y, for the caller's all-gather (fmmbem_plan_assemble_slices_device puts the gathered slices in panel order).
// fold: L2P has stored the result at y[perm[i]] already
int fmmbem_plan::deliver(const DevicePlan& dv, double* d_y, bool fold, hipStream_t s) const {
  if (fold) return FMMBEM_OK;
  if (result_slices) {
    HIP_TRY(hipMemcpyAsync(d_y, dv.yt + dv.row_begin * dv.dof, sizeof(double) * (size_t)(dv.row_end - dv.row_begin) * dv.dof,
                           hipMemcpyDeviceToDevice, s));
  } else if (targets) {                                // the target rows -> distinct points -> the targets as given
    HIP_TRY(launch_scatter_y(dv, d_target_point ? y_points : d_y, s));
    if (d_target_point) {
      const int64_t nt = hp.n_targets * dv.dof;
      hipLaunchKernelGGL(expand_targets_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, d_target_point, y_points, d_y, nt, dv.dof);
      HIP_TRY(hipGetLastError());
    }
  } else {
    if (hp.opt.shard_world > 1) HIP_TRY(hipMemsetAsync(d_y, 0, sizeof(double) * (size_t)hp.n * dv.dof, s));
    HIP_TRY(launch_scatter_y(dv, d_y, s));
  }
  return FMMBEM_OK;
}

// The near field of the potential into y_tree, by the kernel the plan's options pick: what run() and the flow execute launch
int fmmbem_plan::near_potential(bool near_f32, hipStream_t ns) {
  // a target plan: rows of target leaves without a near pair (targets away from the surface) are not written by the near field,
  // only added to by L2P -- they start from zero
  if (targets && zero_target_rows)
    HIP_TRY(hipMemsetAsync(d.yt + hp.n_src * d.dof, 0, sizeof(double) * (size_t)(hp.n - hp.n_src) * d.dof, ns));
  if (g.hybrid) HIP_TRY(launch_near_hybrid(d, ns, hyb));
  else if (near_f32) HIP_TRY(launch_near_spmv_f32(d, ns));        // the float copy at the low orders (near_f32_max_p)
  else if (opts.sparse_local) HIP_TRY(launch_near_spmv(d, ns)); else HIP_TRY(launch_near_matfree(d, ns));
  return FMMBEM_OK;
}

int fmmbem_plan::run(int p, const double* d_x, double* d_y, hipStream_t s, bool near_only, Phase phase, double* xbuf) {
  if (!on_device && targets) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  if (!on_device) return fail(FMMBEM_ERR_NO_DEVICE, "plan was built host-only; there is no CPU execution path");
  if (p < 1 || p > hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  const bool whole = phase == Phase::Whole, takes_x = whole || phase == Phase::Upward;
  if ((takes_x && !d_x) || (phase != Phase::Upward && !d_y)) return fail(FMMBEM_ERR_INVALID, "null vector");
  if (g.split_upward && whole && !near_only)
    return fail(FMMBEM_ERR_UNSUPPORTED, "plan shards the upward pass: use fmmbem_plan_upward_device / _downward_device");
  if (!whole && (!g.split_upward || (!xbuf && phase != Phase::NearSplit))) return fail(FMMBEM_ERR_INVALID, "split execute needs shard_upward and an exchange buffer");
  if (targets && (!whole || result_slices)) return fail(FMMBEM_ERR_UNSUPPORTED, "a target plan runs whole executes only");
  DEVICE_SCOPE(opts.device);
  const int64_t ring = ev_count % kRing;
  StageMarks tm{timing, timing ? &ev[(size_t)ring * 2 * kStages] : nullptr, takes_x ? 0 : pending_mask};
  // Stage order of the reference (EvalInteractionLazySparse.hpp:120-168): near-field SpMV, then P2M, M2M, M2L, L2L, L2P, all on
  // the caller's stream.  (The near field on a second stream beside the far field was measured in rounds 1, 2 and 3 in five
  // variants and is slower every time -- beside the saturated memory system of the near field every dependent access of the
  // latency-bound far kernels takes 10-70x longer; profiles/r03d_overlap_near_far.txt, DESIGN.md section 9 -- and is gone.)
  // a region of the chain, launch by launch or as a graph (see GraphEntry)
  const bool graph_ok = use_graphs && timing == 0;
  auto graphed = [&](int region, const void* buf, auto&& body) -> int {
    if (!graph_ok) return body(s);
    GraphEntry* ge = nullptr;
    for (auto& g : graphs) if (g.region == region && g.p == p && g.buf == buf) ge = &g;
    if (!ge) { graphs.push_back(GraphEntry{region, p, buf, 0, nullptr}); ge = &graphs.back(); }
    if (++ge->runs == 1) return body(s);
    if (!ge->exec) {
      // one capture at a time in the process: the shards of a device list are issued by threads of their own, and a capture on one
      // thread made another thread's hipStreamWaitEvent fail ("dependency created on uncaptured work in another stream")
      static std::mutex capture_mu;
      std::lock_guard<std::mutex> capture_lock(capture_mu);
      HIP_TRY(hipStreamBeginCapture(own_stream, hipStreamCaptureModeThreadLocal));
      const int rc = body(own_stream);
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(own_stream, &g);
      if (rc != FMMBEM_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
      HIP_TRY(e);
      const hipError_t ei = hipGraphInstantiate(&ge->exec, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIP_TRY(ei);
    }
    HIP_TRY(hipGraphLaunch(ge->exec, s));
    return FMMBEM_OK;
  };
  if (takes_x) {
    HIP_TRY(tm.begin(Stage::Gather, s));
    DevicePlan dg = d;
    if (targets) dg.n = hp.n_src;                      // x: the source panels only (the target rows of x_tree stay 0)
    HIP_TRY(launch_gather_x(dg, d_x, s));
    HIP_TRY(tm.end(Stage::Gather, s));
  }
  if (phase == Phase::Upward) {                        // upward half: my leaves, my boxes, pack what the others need
    TRY(graphed(kRegionUpward, xbuf, [&](hipStream_t s) -> int {
      TRY(p2m(d, p, tm, s));
      HIP_TRY(tm.begin(Stage::M2M, s));
      TRY(shift_pass(d, p, ShiftDir::Up, s));
      HIP_TRY(launch_xch_pack(d, p, reinterpret_cast<double2*>(xbuf), s));
      HIP_TRY(tm.end(Stage::M2M, s));
      return FMMBEM_OK;
    }));
    pending_mask = tm.mask;
    pending_near = false;
    return FMMBEM_OK;
  }
  const bool near_f32 = d.near_f32 && p <= opts.near_f32_max_p;
  auto near_field = [&](hipStream_t ns) -> int {
    HIP_TRY(tm.begin(Stage::Spmv, ns));
    TRY(near_potential(near_f32, ns));
    HIP_TRY(tm.end(Stage::Spmv, ns));
    return FMMBEM_OK;
  };
  const bool fold = l2p_delivers(near_only, phase);  // L2P stores into d_y: the scatter stage then brackets nothing
  if (phase == Phase::NearSplit) {                     // the near field of a split execute, while the caller's all-gather is in flight
    TRY(near_field(s));
    pending_mask = tm.mask;
    pending_near = true;
    return FMMBEM_OK;
  }
  const bool near_here = !(phase == Phase::Downward && pending_near);
  pending_near = false;
  // The near field and P2M as ONE launch (launch_near_p2m: the P2M workgroups start where the near field's retire) on a whole
  // execute whose near field is near_spmv_pipe_kernel and whose P2M is p2m_stream_kernel.  Stage timing keeps the two launches:
  // its events bracket the near kernel alone.  FMMBEM_NEAR_P2M, read per launch: 0 = separate launches, 2 = one launch or
  // FMMBEM_ERR_UNSUPPORTED (tests: proves which path ran), otherwise one launch where eligible.
  const int fuse_mode = sw::near_p2m();
  const bool fuse = fuse_mode != 0 && whole && !near_only && !targets && !treecode() && timing == 0 && !g.hybrid && !near_f32 && opts.sparse_local &&
                    d.kernel != FMMBEM_KERNEL_STOKES_BEM && near_p2m_ok(d, p);
  if (fuse_mode == 2 && !fuse) return fail(FMMBEM_ERR_UNSUPPORTED, "FMMBEM_NEAR_P2M=2: this execute does not take the combined near-field / P2M launch");
  const int region = (phase == Phase::Downward ? kRegionDownward : 0) | (near_here ? 0 : kRegionNearDone) | (near_only ? kRegionNearOnly : 0) |
                     (fold ? kRegionFold : 0) | (fuse ? kRegionFused : 0);
  // L2P's folded store takes the caller's pointer: a graph leaves it out, and it follows the replay, as the scatter does
  const L2PTo to = !fold ? L2PTo::YTree : graph_ok ? L2PTo::Caller : L2PTo::Perm;
  TRY(graphed(region, xbuf, [&](hipStream_t s) -> int {
    if (fuse) HIP_TRY(launch_near_p2m(d, p, s));
    else if (near_here) TRY(near_field(s));
    if (near_only) return FMMBEM_OK;
    if (whole && !fuse) TRY(p2m(d, p, tm, s));
    return far_chain(d, d_dev, p, whole, whole ? nullptr : xbuf, to, d_y, tm, s);       // (Downward: the other shards' multipoles in xbuf)
  }));
  if (to == L2PTo::Caller) TRY(l2p(d, p, d_y, s));
  HIP_TRY(tm.begin(Stage::Scatter, s));
  TRY(deliver(d, d_y, fold, s));
  HIP_TRY(tm.end(Stage::Scatter, s));
  last_p = p;
  last_near_f32 = near_f32 ? 1 : 0;
  if (timing) { ev_mask[ring] = tm.mask; ++ev_count; }
  return FMMBEM_OK;
}

// ======================================= field quantities =======================================
// What the four field executes differ in (include/fmmbem.h "Field gradient", "Field pressure", "Field velocity gradient", "Field
// Hessian"): the
// doubles per target, the plans a quantity accepts and the texts of its refusals, the doubles per pair and the most pairs of its
// fmmbem_kernel_*_entries call.  Indexed by FieldQuantity, as the plan's buffers and the launchers of kernels_field.hip are.
struct FieldRow {
  int width;
  bool stokes;                                         // Stokes plans only / Laplace plans only
  const char *needs_targets, *needs_kernel;
  const char* no_double_layer;                         // VELOCITY targets only; null: the target's flag picks the integrand
  int entry_width;
  size_t max_pairs;
  const char* entries_kernel;
  int l2p_from = 1;                                    // the lowest order at which the quantity's L2P has a term: below it no L2P stage
};
static const FieldRow kField[4] = {
    {3, false, "the field gradient: on a plan over separate targets only (fmmbem_plan_create_targets, _create_field)",
     "the field gradient: Laplace plans only", nullptr, 3, (size_t)1 << 30, "the field gradient: the Laplace kernel only"},
    {1, true, "the field pressure: on a plan over separate targets only (fmmbem_plan_create_field)", "the field pressure: Stokes plans only",
     "the field pressure: VELOCITY targets only (the pressure of the double layer is not built)", 3, (size_t)1 << 30,
     "the field pressure: the Stokes kernel only"},
    {9, true, "the field velocity gradient: on a plan over separate targets only (fmmbem_plan_create_field)",
     "the field velocity gradient: Stokes plans only",
     "the field velocity gradient: VELOCITY targets only (the gradient of the double layer is not built)", 27, (size_t)1 << 26,
     "the field velocity gradient: the Stokes kernel only", 2},
    {9, false, "the field Hessian: on a plan over separate targets only (fmmbem_plan_create_targets, _create_field)",
     "the field Hessian: Laplace plans only", nullptr, 9, (size_t)1 << 27, "the field Hessian: the Laplace kernel only", 2},
};

// the refusals of a field execute after the null checks, in the order include/fmmbem.h states them
int fmmbem_plan::field_refusal(FieldQuantity q, int p) const {
  const FieldRow& row = kField[(int)q];
  if (p < 1 || p > hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  if (!targets) return fail(FMMBEM_ERR_UNSUPPORTED, row.needs_targets);
  if ((opts.kernel == FMMBEM_KERNEL_STOKES_BEM) != row.stokes) return fail(FMMBEM_ERR_UNSUPPORTED, row.needs_kernel);
  if (row.no_double_layer && has_bc[1]) return fail(FMMBEM_ERR_UNSUPPORTED, row.no_double_layer);
  if (!on_device) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  return FMMBEM_OK;
}

int fmmbem_plan::field_alloc(FieldQuantity q) {
  const size_t rows = (size_t)(hp.n - hp.n_src), w = (size_t)kField[(int)q].width;
  FieldBuffers& b = field[(int)q];
  if (!b.tree) TRY(alloc(w * rows, &b.tree, false));
  if (d_target_point && !b.points) TRY(alloc(w * rows, &b.points, false));
  if (!b.stage) TRY(alloc(w * (size_t)hp.n_targets, &b.stage, false));
  return FMMBEM_OK;
}

// A field execute: run()'s gather, P2M and far chain up to and including L2L on the plan's own M and L -- the same launches in the
// same order, so the same L -- then the quantity's two kernels of kernels_field.hip into its tree buffer and the delivery.
// Launched plainly (never captured, never replayed; `graphs` is not touched), it writes x_tree, M, Mh and L, which every potential
// execute writes afresh before it reads them, and leaves y_tree alone.
int fmmbem_plan::run_field(FieldQuantity q, int p, const double* d_x, double* d_out, hipStream_t s) {
  if (!d_x || !d_out) return fail(FMMBEM_ERR_INVALID, "null vector");
  TRY(field_refusal(q, p));
  DEVICE_SCOPE(opts.device);
  TRY(field_alloc(q));
  const FieldBuffers& b = field[(int)q];
  const int64_t ring = ev_count % kRing;
  StageMarks tm{timing, timing ? &ev[(size_t)ring * 2 * kStages] : nullptr, 0};
  HIP_TRY(tm.begin(Stage::Gather, s));
  DevicePlan dg = d;
  dg.n = hp.n_src;                                     // x: the source panels only (the target rows of x_tree stay 0)
  HIP_TRY(launch_gather_x(dg, d_x, s));
  HIP_TRY(tm.end(Stage::Gather, s));
  TRY(p2m(d, p, tm, s));
  TRY(far_chain(d, d_dev, p, true, nullptr, L2PTo::Caller, nullptr, tm, s));      // (Caller: no L2P in there)
  HIP_TRY(tm.begin(Stage::Spmv, s));
  HIP_TRY(launch_near_field(q, d, hp.n_src, b.tree, s));
  HIP_TRY(tm.end(Stage::Spmv, s));
  if (p >= kField[(int)q].l2p_from) {
    HIP_TRY(tm.begin(Stage::L2P, s));
    HIP_TRY(launch_l2p_field(q, d, p, hp.n_src, b.tree, s));
    HIP_TRY(tm.end(Stage::L2P, s));
  } else {
    tm.mask &= ~(1u << (int)Stage::L2P);               // nothing is launched: far_chain's empty pair does not count, ms_l2p = 0
  }
  HIP_TRY(tm.begin(Stage::Scatter, s));
  TRY(deliver_field(q, d_out, s));
  HIP_TRY(tm.end(Stage::Scatter, s));
  last_p = p;
  if (timing) { ev_mask[ring] = tm.mask; ++ev_count; }
  return FMMBEM_OK;
}

// a quantity's tree buffer -> the distinct points -> the targets as given
int fmmbem_plan::deliver_field(FieldQuantity q, double* d_out, hipStream_t s) const {
  const int width = kField[(int)q].width;
  const FieldBuffers& b = field[(int)q];
  HIP_TRY(launch_field_scatter(q, d, hp.n_src, b.tree, d_target_point ? b.points : d_out, s));
  if (d_target_point) {
    const int64_t nu = width * (int64_t)hp.n_targets;  // unknowns, one thread each
    hipLaunchKernelGGL(expand_targets_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s, d_target_point, b.points, d_out, nu, width);
    HIP_TRY(hipGetLastError());
  }
  return FMMBEM_OK;
}

// ======================================= representation execute =======================================
// fmmbem_plan_execute_representation: phi = S[sigma] - D[mu] and its gradient at the points of a Laplace target plan, the targets'
// own flags ignored.  Both layers are Laplace expansions about the same centres moved by the same operators, so they are FOLDED
// into one multipole set at the leaves: P2M per layer into its own slot of M (the per-slot views of p2m_targets: every source taken
// with the slot's flag, the slot's table, the layer's vector), then M_slot0 += M_slot1 at the P2M leaves, and ONE far chain on a
// one-slot view (n_act = 1, act[0] = 0, every row's flag 0).  The signs: l2p_kernel adds +r0 at a flag-0 target and -r1 at a
// flag-1 target, so S - D has the far field r0 + r1 -- the value and the gradient of the expansion L0 + L1, which is the L of
// M0 + M1.  M is addressed by the slot's NUMBER (act[a]), not by its position among the live slots, and both slots of a Laplace
// plan exist whatever its targets' flags: the second P2M lands beside the first, never on it.
// Launched plainly like a field execute.  It writes x_tree, both slots of M at the leaves, and slot 0 of M, Mh and L above them;
// every potential execute writes what it reads of these afresh, and y_tree is left alone.
int fmmbem_plan::representation_refusal(int p) const {
  if (p < 1 || p > hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  if (!targets) return fail(FMMBEM_ERR_UNSUPPORTED, "the representation execute: on a plan over separate targets only (fmmbem_plan_create_targets, _create_field)");
  if (opts.kernel == FMMBEM_KERNEL_STOKES_BEM) return fail(FMMBEM_ERR_UNSUPPORTED, "the representation execute: Laplace plans only");
  if (!on_device) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  if (treecode()) return fail(FMMBEM_ERR_UNSUPPORTED, "the representation execute: FMM plans only (the treecode has no local expansions)");
  return FMMBEM_OK;
}

// the plan with slot 0 alone live and every row a flag-0 row: what the far chain, L2P and the gradient's L2P run on
DevicePlan fmmbem_plan::representation_view() const {
  DevicePlan v = d;
  v.n_act = 1; v.act[0] = 0;
  v.bc = bc_all[0];
  if (d.p2m_tab) v.p2m_tab = p2m_tab_slot[0];
  return v;
}

// Buffers of the representation execute, each at its first use; a failure leaves what was allocated in place for the next call
int fmmbem_plan::representation_alloc(bool value, bool gradient) {
  const size_t rows = (size_t)(hp.n - hp.n_src);
  bool zeroed = false;
  if (!rep.mu_tree) { TRY(alloc((size_t)hp.n, &rep.mu_tree, true)); zeroed = true; }
  if (!rep.stage_mu) TRY(alloc((size_t)hp.n_src, &rep.stage_mu, false));
  if (value) {
    if (!rep.phi_tree) { TRY(alloc((size_t)hp.n, &rep.phi_tree, true)); zeroed = true; }
    if (d_target_point && !rep.phi_points) TRY(alloc(rows, &rep.phi_points, false));
    if (!rep.phi_stage) TRY(alloc((size_t)hp.n_targets, &rep.phi_stage, false));
  }
  if (gradient) TRY(field_alloc(FieldQuantity::Gradient));
  // the moment table of a slot the plan's own targets do not make live (the plan's own P2M without tables: this one too)
  for (int f = 0; d.p2m_tab && f < 2; ++f)
    if (!p2m_tab_slot[f]) TRY(p2m_table(bc_all[f], &p2m_tab_slot[f]));
  if (!rep.view_dev) {
    const DevicePlan v = representation_view();
    TRY(allocs.upload(&v, 1, &rep.view_dev));
  }
  if (zeroed) HIP_TRY(hipDeviceSynchronize());         // the zero-fills ran on the NULL stream
  return FMMBEM_OK;
}

int fmmbem_plan::run_representation(int p, const double* d_sigma, const double* d_mu, double* d_phi, double* d_grad, hipStream_t s) {
  if ((!d_sigma && !d_mu) || (!d_phi && !d_grad)) return fail(FMMBEM_ERR_INVALID, "no layer given, or no output asked");
  TRY(representation_refusal(p));
  DEVICE_SCOPE(opts.device);
  TRY(representation_alloc(d_phi != nullptr, d_grad != nullptr));
  const DevicePlan v = representation_view();
  double* const pt = d_phi ? rep.phi_tree + hp.n_src : nullptr;                   // the target rows of the value's tree buffer
  double* const gt = d_grad ? field[(int)FieldQuantity::Gradient].tree : nullptr;
  const int64_t ring = ev_count % kRing;
  StageMarks tm{timing, timing ? &ev[(size_t)ring * 2 * kStages] : nullptr, 0};
  // sigma into x_tree, mu into the second buffer, source rows only; a layer that is not given is a zero vector to the near kernel
  HIP_TRY(tm.begin(Stage::Gather, s));
  const double* const layer[2] = {d_sigma, d_mu};
  double* const layer_tree[2] = {d.xt, rep.mu_tree};
  for (int f = 0; f < 2; ++f) {
    DevicePlan dg = d;
    dg.n = hp.n_src;
    dg.xt = layer_tree[f];
    if (layer[f]) HIP_TRY(launch_gather_x(dg, layer[f], s));
    else HIP_TRY(hipMemsetAsync(layer_tree[f], 0, sizeof(double) * (size_t)hp.n_src, s));
  }
  HIP_TRY(tm.end(Stage::Gather, s));
  // P2M per layer given (p2m_targets' views), then the fold; a layer that is not given has no P2M
  HIP_TRY(tm.begin(Stage::P2M, s));
  for (int f = 0; f < 2; ++f) {
    if (!layer[f]) continue;
    DevicePlan dp = d;
    dp.bc = bc_all[f];
    dp.n_act = 1; dp.act[0] = f;
    dp.xt = layer_tree[f];
    if (d.p2m_tab) dp.p2m_tab = p2m_tab_slot[f];
    HIP_TRY(launch_p2m(dp, p, s));
  }
  if (d_mu) HIP_TRY(launch_fold_slots(d, p, /*set=*/!d_sigma, s));
  HIP_TRY(tm.end(Stage::P2M, s));
  TRY(far_chain(v, rep.view_dev, p, true, nullptr, L2PTo::Caller, nullptr, tm, s));          // (Caller: no L2P in there)
  HIP_TRY(tm.begin(Stage::Spmv, s));
  HIP_TRY(launch_near_representation(d, hp.n_src, rep.mu_tree, pt, gt, s));
  HIP_TRY(tm.end(Stage::Spmv, s));
  HIP_TRY(tm.begin(Stage::L2P, s));
  if (d_phi) HIP_TRY(launch_l2p(v, p, rep.phi_tree, s));
  if (d_grad) HIP_TRY(launch_l2p_field(FieldQuantity::Gradient, v, p, hp.n_src, gt, s));
  HIP_TRY(tm.end(Stage::L2P, s));
  HIP_TRY(tm.begin(Stage::Scatter, s));
  if (d_phi) {
    HIP_TRY(launch_value_scatter(d, hp.n_src, pt, d_target_point ? rep.phi_points : d_phi, s));
    if (d_target_point) {
      const int64_t nu = hp.n_targets;
      hipLaunchKernelGGL(expand_targets_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s, d_target_point, rep.phi_points, d_phi, nu, 1);
      HIP_TRY(hipGetLastError());
    }
  }
  if (d_grad) TRY(deliver_field(FieldQuantity::Gradient, d_grad, s));
  HIP_TRY(tm.end(Stage::Scatter, s));
  last_p = p;
  if (timing) { ev_mask[ring] = tm.mask; ++ev_count; }
  return FMMBEM_OK;
}

// ======================================= flow execute =======================================
// fmmbem_plan_execute_flow: what the velocity execute and the pressure's and the velocity gradient's field executes write, on ONE
// gather, P2M and far chain.  Every kernel that touches an output is the one the single execute launches, on the same L, in the
// same order per buffer -- near kernel, then L2P, then the delivery -- so each output has the single execute's bits; the one new
// kernel, near_flow_kernel (kernels_field.hip), writes the pressure's and the gradient's tree buffers with their own kernels' bits.
// Launched plainly like a field execute; the velocity's near field goes into y_tree as run() puts it there (near_potential).
int fmmbem_plan::flow_refusal(int p) const {
  if (p < 1 || p > hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  if (!targets) return fail(FMMBEM_ERR_UNSUPPORTED, "the flow execute: on a plan over separate targets only (fmmbem_plan_create_field)");
  if (opts.kernel != FMMBEM_KERNEL_STOKES_BEM) return fail(FMMBEM_ERR_UNSUPPORTED, "the flow execute: Stokes plans only");
  if (has_bc[1]) return fail(FMMBEM_ERR_UNSUPPORTED, "the flow execute: VELOCITY targets only (the pressure and the gradient of the double layer are not built)");
  if (!on_device) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  return FMMBEM_OK;
}

int fmmbem_plan::run_flow(int p, const double* d_x, double* d_u, double* d_q, double* d_G, hipStream_t s) {
  if (!d_x || (!d_u && !d_q && !d_G)) return fail(FMMBEM_ERR_INVALID, "null vector, or no output asked");
  TRY(flow_refusal(p));
  DEVICE_SCOPE(opts.device);
  if (d_q) TRY(field_alloc(FieldQuantity::Pressure));
  if (d_G) TRY(field_alloc(FieldQuantity::VelocityGradient));
  double* const qt = field[(int)FieldQuantity::Pressure].tree;
  double* const gt = field[(int)FieldQuantity::VelocityGradient].tree;
  const int64_t ring = ev_count % kRing;
  StageMarks tm{timing, timing ? &ev[(size_t)ring * 2 * kStages] : nullptr, 0};
  HIP_TRY(tm.begin(Stage::Gather, s));
  DevicePlan dg = d;
  dg.n = hp.n_src;                                     // x: the source panels only (the target rows of x_tree stay 0)
  HIP_TRY(launch_gather_x(dg, d_x, s));
  HIP_TRY(tm.end(Stage::Gather, s));
  TRY(p2m(d, p, tm, s));
  TRY(far_chain(d, d_dev, p, true, nullptr, L2PTo::Caller, nullptr, tm, s));      // (Caller: no L2P in there)
  const bool near_f32 = d.near_f32 && p <= opts.near_f32_max_p;                   // as run() picks the velocity's near kernel
  HIP_TRY(tm.begin(Stage::Spmv, s));
  if (d_u) TRY(near_potential(near_f32, s));
  if (d_q && d_G) HIP_TRY(launch_near_flow(d, hp.n_src, qt, gt, s));
  else if (d_q) HIP_TRY(launch_near_field(FieldQuantity::Pressure, d, hp.n_src, qt, s));
  else if (d_G) HIP_TRY(launch_near_field(FieldQuantity::VelocityGradient, d, hp.n_src, gt, s));
  HIP_TRY(tm.end(Stage::Spmv, s));
  HIP_TRY(tm.begin(Stage::L2P, s));
  if (d_u) TRY(l2p(d, p, nullptr, s));
  if (d_q) HIP_TRY(launch_l2p_field(FieldQuantity::Pressure, d, p, hp.n_src, qt, s));
  if (d_G) HIP_TRY(launch_l2p_field(FieldQuantity::VelocityGradient, d, p, hp.n_src, gt, s));
  HIP_TRY(tm.end(Stage::L2P, s));
  HIP_TRY(tm.begin(Stage::Scatter, s));
  if (d_u) TRY(deliver(d, d_u, false, s));
  if (d_q) TRY(deliver_field(FieldQuantity::Pressure, d_q, s));
  if (d_G) TRY(deliver_field(FieldQuantity::VelocityGradient, d_G, s));
  HIP_TRY(tm.end(Stage::Scatter, s));
  last_p = p;
  last_near_f32 = d_q && d_G ? kFlowNearFused : d_q || d_G ? kFlowNearSingle : kFlowNearNone;
  if (timing) { ev_mask[ring] = tm.mask; ++ev_count; }
  return FMMBEM_OK;
}

// ======================================= batched execute =======================================
// Vectors per near-field pass on the fast path (FMMBEM_BATCH_NV = 2, 4 or 8 for sweeps).  ms per vector at N = 1M, k = 4 / 8,
// p = 10 and 2 (tools/batch_time.py, profiles/r06b_batch_time.txt): 2 -> 1.24, 0.59; 4 -> 1.16, 0.56; 8 -> 1.29, 0.67.
// the plans whose near field is the pipelined one-unknown SpMV on one device (include/fmmbem.h, fmmbem_plan_execute_batch), and
// the Stokes plans with the symmetric blocks that ask for it (fmmbem_options.stokes_batch_width)
int fmmbem_plan::batch_width() const {
  const bool one = on_device && !multi && opts.sparse_local && !g.hybrid && hp.opt.shard_world <= 1 && !g.split_upward && !result_slices &&
                   !d.near_f32;                      // float near field: vector by vector, each with the bits of its single execute
  if (!one) return 1;
  if (opts.kernel == FMMBEM_KERNEL_STOKES_BEM)
    return !targets && opts.stokes_batch_width >= 2 && batch_near_sym3_ok(d, opts.stokes_batch_width) ? opts.stokes_batch_width : 1;
  return !batch_near_ok(d) ? 1 : bat.width ? bat.width : sw::batch_nv();
}

// all or nothing: a failed allocation leaves the plan as it was (FMMBEM_ERR_ALLOC; single executes are unaffected)
int fmmbem_plan::batch_alloc(hipStream_t s) {
  if (bat.width) return FMMBEM_OK;
  const int w = opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? opts.stokes_batch_width : sw::batch_nv();
  const size_t nt = (size_t)hp.n * d.dof, nm = (size_t)hp.nboxes * d.nslots * d.s_max;
  BatchBufs b;
  std::vector<void*> got;
  auto get = [&](size_t bytes, auto** out) -> bool {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(bytes, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
    got.push_back(q);
    *out = static_cast<std::remove_pointer_t<decltype(out)>>(q);
    return true;
  };
  bool ok = true;
  for (int j = 0; j < w && ok; ++j)
    ok = get(nt * sizeof(double), &b.xt[j]) && get(nt * sizeof(double), &b.yt[j]) && get(nm * sizeof(double2), &b.M[j]) &&
         get(sizeof(DevicePlan), &b.dev[j]);
  for (int j = 0; j < w && ok; ++j) {
    // zero as the plan's own x_tree, y_tree and M (a target plan's x rows of the targets stay 0); on `s`, ahead of the batch
    ok = hipMemsetAsync(b.xt[j], 0, nt * sizeof(double), s) == hipSuccess && hipMemsetAsync(b.yt[j], 0, nt * sizeof(double), s) == hipSuccess &&
         hipMemsetAsync(b.M[j], 0, nm * sizeof(double2), s) == hipSuccess;
    const DevicePlan dj = batch_view(b, j);
    ok = ok && hipMemcpy(b.dev[j], &dj, sizeof(DevicePlan), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipStreamSynchronize(s);
    for (void* q : got) (void)hipFree(q);
    (void)hipGetLastError();
    return fail(FMMBEM_ERR_ALLOC, "batch buffers: device allocation failed");
  }
  for (void* q : got) allocs.list.push_back(q);           // this plan's alone, freed at destroy
  b.width = w;
  bat = b;
  return FMMBEM_OK;
}

// The fast path: per pass of up to bat.width vectors the gathers, ONE near-field pass and one P2M pass (launch_near_spmv_multi,
// launch_p2m_multi; a Stokes plan: launch_near_sym3_multi, and P2M with the single launcher per vector: there is no batched far
// field), then run()'s far chain (far_chain) and the delivery once per vector, on d pointing at that vector's buffers: the same
// bits.  host: x and y are host pointers, staged through stage_x / stage_y(_targets) one vector at a time, in stream order.
// With stage timing on, each pass records its near-field and P2M passes (fmmbem_plan_stats ms_near, ms_p2m: means per pass).
int fmmbem_plan::run_batch(int p, int k, const double* x, size_t ldx, double* y, size_t ldy, hipStream_t s, bool host) {
  if (p < 1 || p > hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  DEVICE_SCOPE(opts.device);
  TRY(batch_alloc(s));
  const int w = bat.width;
  const bool stokes = d.dof == 3;                      // never a target plan (batch_width)
  const size_t bytes_x = sizeof(double) * x_doubles(), bytes_y = sizeof(double) * y_doubles();
  double* sy = targets ? stage_y_targets : stage_y;
  StageMarks no_marks;                                 // a vector's far chain records nothing
  BatchVecs bv{};
  bv.width = w;
  for (int j = 0; j < w; ++j) { bv.xt[j] = bat.xt[j]; bv.yt[j] = bat.yt[j]; bv.M[j] = bat.M[j]; }
  for (int j0 = 0; j0 < k; j0 += w) {
    const int nv = std::min(w, k - j0);
    bv.nv = nv;
    for (int j = 0; j < nv; ++j) {
      const double* xj = x + (size_t)(j0 + j) * ldx;
      if (host) { HIP_TRY(hipMemcpyAsync(stage_x, xj, bytes_x, hipMemcpyHostToDevice, s)); xj = stage_x; }
      DevicePlan dg = d;
      dg.xt = bat.xt[j];
      if (targets) dg.n = hp.n_src;                  // the target rows of x_tree stay 0
      HIP_TRY(launch_gather_x(dg, xj, s));
      if (targets && zero_target_rows)
        HIP_TRY(hipMemsetAsync(bat.yt[j] + hp.n_src * d.dof, 0, sizeof(double) * (size_t)(hp.n - hp.n_src) * d.dof, s));
    }
    // stage timing on (either mode): a pass is one record of the ring with two stages, its near-field pass and its P2M; a Stokes
    // pass records its near-field pass alone (P2M runs per vector, below)
    StageMarks pass{timing ? 1 : 0, timing ? &ev[(size_t)(ev_count % kRing) * 2 * kStages] : nullptr};
    HIP_TRY(pass.begin(Stage::Spmv, s));
    if (stokes) HIP_TRY(launch_near_sym3_multi(d, bv, s)); else HIP_TRY(launch_near_spmv_multi(d, bv, s));
    HIP_TRY(pass.end(Stage::Spmv, s));
    if (!stokes) {
      HIP_TRY(pass.begin(Stage::P2M, s));
      if (targets) TRY(p2m_targets(d, [&](const DevicePlan& dp) { return launch_p2m_multi(dp, bv, p, s); }));
      else HIP_TRY(launch_p2m_multi(d, bv, p, s));
      HIP_TRY(pass.end(Stage::P2M, s));
    }
    if (timing) { ev_mask[ev_count % kRing] = pass.mask; ++ev_count; }
    for (int j = 0; j < nv; ++j) {
      double* yj = host ? sy : y + (size_t)(j0 + j) * ldy;
      const DevicePlan dj = batch_view(bat, j);        // vector j's far field: run()'s chain on its buffers and its device copy
      if (stokes) TRY(p2m(dj, p, no_marks, s));
      const bool fold = l2p_delivers(false, Phase::Whole);
      TRY(far_chain(dj, bat.dev[j], p, true, nullptr, fold ? L2PTo::Perm : L2PTo::YTree, yj, no_marks, s));
      TRY(deliver(dj, yj, fold, s));
      if (host) HIP_TRY(hipMemcpyAsync(y + (size_t)(j0 + j) * ldy, sy, bytes_y, hipMemcpyDeviceToHost, s));
    }
  }
  if (host) HIP_TRY(hipStreamSynchronize(s));
  last_p = p;
  return FMMBEM_OK;
}

// ============================================ C ABI ============================================
extern "C" {

void fmmbem_options_default(fmmbem_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->kernel = FMMBEM_KERNEL_LAPLACE_BEM;
  o->p_max = 10;
  o->quad_k = 3;
  o->theta = 0.5;
  o->ncrit = 64;
  o->sparse_local = 1;
  o->shard_world = 1;
  o->quad_k_fine = 25;          // StokesSphericalBEM ctor default (kernel/StokesSphericalBEM.hpp:131)
  o->mu = 1e-3;
  o->near_stream_fraction = 1.0;
  o->near_f32_max_p = 0;
  o->stokes_batch_width = 0;
}

// ---- plans that share a geometry -----------------------------------------------------------------------------
// Two independent 64-bit hashes of the vertex bytes (the panels in the caller's order), a few threads: 75 MB at N = 1M in ~5 ms
static void fingerprint_vertices(const double* v, size_t n_panels, uint64_t out[2]) {
  const size_t words = n_panels * 9;
  const int nt = words < (1u << 20) ? 1 : (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<uint64_t> part((size_t)nt * 2);
  auto work = [&](int t) {
    const size_t w0 = words * t / nt, w1 = words * (t + 1) / nt;
    uint64_t a = 0x9E3779B97F4A7C15ull + t, b = 0xC2B2AE3D27D4EB4Full ^ (uint64_t)t;
    for (size_t i = w0; i < w1; ++i) {
      uint64_t x;
      std::memcpy(&x, v + i, 8);
      a = (a ^ x) * 0x100000001B3ull; a ^= a >> 29;                       // FNV-style multiply-xor with a fold
      b += x * 0xFF51AFD7ED558CCDull; b = (b << 27) | (b >> 37); b *= 0xC4CEB9FE1A85EC53ull;
    }
    part[2 * t] = a; part[2 * t + 1] = b;
  };
  if (nt == 1) work(0);
  else {
    host_parallel(nt, [&](int t) { work(t); });
  }
  uint64_t a = n_panels, b = ~(uint64_t)n_panels;
  for (int t = 0; t < nt; ++t) { a = (a ^ part[2 * t]) * 0x100000001B3ull; b = (b + part[2 * t + 1]) * 0xC4CEB9FE1A85EC53ull; b ^= b >> 31; }
  out[0] = a; out[1] = b | 1;                                             // never 0 0
}

// the options that decide the geometry's share of a plan: everything but the flags (and mu, which only scales near values)
static bool same_geometry_options(const fmmbem_options& a, const fmmbem_options& b) {
  return a.kernel == b.kernel && a.p_max == b.p_max && a.quad_k == b.quad_k && a.theta == b.theta && a.ncrit == b.ncrit &&
         a.sparse_local == b.sparse_local && a.host_only == b.host_only && a.device == b.device && a.shard_rank == b.shard_rank &&
         a.shard_world == b.shard_world && a.quad_k_fine == b.quad_k_fine && a.evaluator == b.evaluator && a.mu == b.mu &&
         a.shard_upward == b.shard_upward && a.l2l_rule == b.l2l_rule && a.near_stream_fraction == b.near_stream_fraction &&
         a.near_f32_max_p == b.near_f32_max_p;
}

// the geometries still alive, most recent first (a handful: operator, right-hand side, preconditioner plans).  The cache owns
// nothing: an entry whose last plan is gone has expired and is dropped at the next insertion.  A creation that finds its geometry
// here takes a reference under the mutex and reads only what no plan ever writes (PlanGeometry, the fingerprint): no live plan
// is looked at, so it cannot race with an execute on another handle.
static std::mutex g_cache_mu;
static std::vector<std::weak_ptr<PlanShared>> g_cache;

static void geometry_cache_add(const std::shared_ptr<PlanShared>& sh) {
  std::lock_guard<std::mutex> lock(g_cache_mu);
  g_cache.erase(std::remove_if(g_cache.begin(), g_cache.end(), [](const std::weak_ptr<PlanShared>& w) { return w.expired(); }), g_cache.end());
  g_cache.insert(g_cache.begin(), sh);
  if (g_cache.size() > 32) g_cache.resize(32);
}
static std::shared_ptr<PlanShared> geometry_cache_find(size_t n_panels, const uint64_t fp[2], const fmmbem_options& o) {
  std::lock_guard<std::mutex> lock(g_cache_mu);
  for (const std::weak_ptr<PlanShared>& w : g_cache)
    if (std::shared_ptr<PlanShared> sh = w.lock())
      if ((size_t)sh->geo.gd.n == n_panels && sh->fingerprint[0] == fp[0] && sh->fingerprint[1] == fp[1] && same_geometry_options(sh->geo.opts, o)) return sh;
  return nullptr;
}

// A plan on a geometry that exists (`sh`: a base plan's, or one the cache recognised) with the options `o` and other
// boundary-condition flags: a new plan with its own stream and events, which builds what the flags decide.
int fmmbem_plan::like(std::shared_ptr<PlanShared> sh, const fmmbem_options& o, const uint8_t* bc, fmmbem_plan** out) {
  *out = nullptr;
  const double t0 = now_ms();
  std::unique_ptr<fmmbem_plan> pl(new (std::nothrow) fmmbem_plan(std::move(sh)));
  if (!pl) return fail(FMMBEM_ERR_ALLOC, "plan");
  pl->opts = o;
  TRY(pl->open_device());
  const HostPlan& h = pl->hp;
  std::vector<uint8_t> bc_tree((size_t)h.n, 0);
  for (int64_t i = 0; i < h.n; ++i) {
    const uint8_t f = bc ? (bc[h.perm[(size_t)i]] ? 1 : 0) : 0;
    bc_tree[(size_t)i] = f;
    pl->has_bc[f] = true;
  }
  TRY(pl->to_device_bc(bc_tree.data()));
  pl->build_host_ms = now_ms() - t0 - pl->build_assemble_ms;
  *out = pl.release();
  return FMMBEM_OK;
}

// ---- one plan over several devices of ONE process (fmmbem_options.n_devices > 1; SURVEY.md section 8b "device list") ------
// The reference's drivers build one plan in one process (examples/LaplaceBEM.cpp:209; FMM_plan.hpp:34-43).  This is that plan with
// its target leaves sharded over the devices of the list: the handle owns one SHARD plan per device (the same shards the
// one-process-per-GPU form drives through torch.distributed, distributed.py) and moves the data between them itself --
//   x (on the first device)  -> a copy per device                                 hipMemcpyPeerAsync, one xGMI link each
//   upward pass by the boxes' owners -> the multipoles each shard's lists read     peer copies of fmmbem_plan_exchange_counts' segments
//   downward pass + near field of every shard -> its tree-order slice of y        -> peer copies into ONE buffer on the first device
//   slices -> y in panel order (fmmbem_plan_assemble_slices_device)
// every step on the shard's own stream, ordered by events: the host thread only enqueues.  xGMI is point to point, so plain peer
// copies ARE the collective here (one link per peer, no ring); the same bits as a single plan (shards sum bitwise).
// Not measured on more than one GPU (none has been available to this project); devices = {0, 0, ...} runs the whole path on one.
struct MultiDevice {
  std::vector<std::unique_ptr<fmmbem_plan>> shards;
  std::vector<int> dev;
  std::vector<double*> x, slice;                     // per shard, on its device: the replica of x, the result slice
  double* gathered = nullptr;                        // on dev[0]: world * chunk doubles
  size_t chunk = 0;
  std::vector<int64_t> cut;
  hipEvent_t ev_x = nullptr;
  std::vector<hipEvent_t> ev_up, ev_done;
  bool split = false;
  struct Xch { std::vector<double*> send, recv; std::vector<std::vector<int64_t>> sc, rc; };
  std::map<int, Xch> xch;                            // per order p
  int world() const { return (int)shards.size(); }
  ~MultiDevice() {
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (int r = 0; r < world(); ++r) {
      (void)hipSetDevice(dev[r]);
      if (r < (int)x.size() && x[r]) (void)hipFree(x[r]);
      if (r < (int)slice.size() && slice[r]) (void)hipFree(slice[r]);
      for (auto& kv : xch) { if (kv.second.send[r]) (void)hipFree(kv.second.send[r]); if (kv.second.recv[r]) (void)hipFree(kv.second.recv[r]); }
      if (r < (int)ev_up.size() && ev_up[r]) (void)hipEventDestroy(ev_up[r]);
      if (r < (int)ev_done.size() && ev_done[r]) (void)hipEventDestroy(ev_done[r]);
    }
    if (!dev.empty()) (void)hipSetDevice(dev[0]);
    if (gathered) (void)hipFree(gathered);
    if (ev_x) (void)hipEventDestroy(ev_x);
    (void)hipSetDevice(prev);
    shards.clear();
  }
};

// the handle over the shards of `m`: what the host-pointer execute and the solver need on the first device
static int multi_finish(const fmmbem_options& opts, std::shared_ptr<MultiDevice> m, fmmbem_plan** out) {
  const int W = m->world();
  const fmmbem_plan& s0 = *m->shards[0];
  std::unique_ptr<fmmbem_plan> h(new (std::nothrow) fmmbem_plan(s0.shared));
  if (!h) return fail(FMMBEM_ERR_ALLOC, "plan");
  h->opts = opts;
  const size_t nd = (size_t)s0.hp.n * s0.d.dof;
  m->cut.resize((size_t)W + 1);
  TRY(fmmbem_plan_shard_rows(m->shards[0].get(), m->cut.data()));
  for (int r = 0; r < W; ++r) m->chunk = std::max(m->chunk, (size_t)(m->cut[r + 1] - m->cut[r]) * s0.d.dof);
  m->chunk = std::max<size_t>(m->chunk, 1);
  m->split = s0.g.split_upward;
  m->x.assign(W, nullptr); m->slice.assign(W, nullptr); m->ev_up.assign(W, nullptr); m->ev_done.assign(W, nullptr);
  int prev = 0;
  (void)hipGetDevice(&prev);
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{prev};
  for (int r = 0; r < W; ++r) {
    HIP_TRY(hipSetDevice(m->dev[r]));
    for (int q = 0; q < W; ++q)                        // direct peer copies where the hardware has them (an error here only means "already on" or "not available")
      if (m->dev[q] != m->dev[r]) { if (hipDeviceEnablePeerAccess(m->dev[q], 0) != hipSuccess) (void)hipGetLastError(); }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->x[r]), sizeof(double) * nd));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->slice[r]), sizeof(double) * m->chunk));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_up[r], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_done[r], hipEventDisableTiming));
    m->shards[r]->result_slices = true;
    m->shards[r]->use_graphs = sw::graph(true);   // a shard's chain is short: the host must stay ahead of W of them
  }
  HIP_TRY(hipSetDevice(m->dev[0]));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->gathered), sizeof(double) * m->chunk * (size_t)W));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_x, hipEventDisableTiming));
  h->opts.device = m->dev[0];
  h->on_device = true;
  h->compose_d();                                    // the first shard's geometry, no flag side: the handle reads d.dof and d.n
  h->has_bc[0] = s0.has_bc[0]; h->has_bc[1] = s0.has_bc[1];
  HIP_TRY(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  TRY(h->alloc(nd, &h->stage_x, true));
  TRY(h->alloc(nd, &h->stage_y, true));
  HIP_TRY(hipDeviceSynchronize());
  h->multi = std::move(m);
  *out = h.release();
  return FMMBEM_OK;
}

static int multi_create(const fmmbem_options* opts, const std::vector<int>& devices, size_t n_panels, const double* vertices,
                        const uint8_t* bc, fmmbem_plan** out) {
  const int W = (int)devices.size();
  if (W > 8) return fail(FMMBEM_ERR_UNSUPPORTED, "at most 8 devices per plan");
  if (opts->shard_world > 1) return fail(FMMBEM_ERR_INVALID, "a plan over several devices is the whole operator: shard_world must be 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FMMBEM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU execution path)");
  for (int d_ : devices) if (d_ < 0 || d_ >= ndev) return fail(FMMBEM_ERR_INVALID, "device ordinal out of range in the device list");
  auto m = std::make_shared<MultiDevice>();
  m->dev = devices;
  m->shards.resize(W);
  // the shards are built side by side: each is a plan_create of its own (host lists of the same tree, then its device's share)
  std::vector<int> rc(W, FMMBEM_OK);
  std::vector<std::string> err(W);
  std::vector<std::thread> pool;
  for (int r = 0; r < W; ++r)
    pool.emplace_back([&, r] {
      fmmbem_options o = *opts;
      o.n_devices = 0; o.device = devices[r]; o.shard_rank = r; o.shard_world = W;
      o.shard_upward = opts->shard_upward == 0 ? 0 : 2;            // 0: every device repeats the upward pass; else: owners + selective exchange
      o.shard_upward = sw::multi_upward(o.shard_upward != 0) ? 2 : 0;
      fmmbem_plan* p = nullptr;
      rc[r] = fmmbem_plan_create(&o, n_panels, vertices, bc, &p);
      if (rc[r] != FMMBEM_OK) err[r] = g_last_error;
      m->shards[r].reset(p);
    });
  for (auto& th : pool) th.join();
  for (int r = 0; r < W; ++r) if (rc[r] != FMMBEM_OK) return fail(rc[r], "shard " + std::to_string(r) + ": " + err[r]);
  return multi_finish(*opts, m, out);
}

// a multi-device plan of `base`'s panels with other flags: shard by shard (each shares its base shard's geometry)
static int multi_like(const fmmbem_plan& base, const uint8_t* bc, fmmbem_plan** out) {
  auto m = std::make_shared<MultiDevice>();
  m->dev = base.multi->dev;
  const int W = base.multi->world();
  m->shards.resize(W);
  for (int r = 0; r < W; ++r) {
    fmmbem_plan* p = nullptr;
    const fmmbem_plan& sb = *base.multi->shards[r];
    TRY(fmmbem_plan::like(sb.shared, sb.opts, bc, &p));
    m->shards[r].reset(p);
  }
  return multi_finish(base.opts, m, out);
}

static int multi_xch(fmmbem_plan* h, int p, MultiDevice::Xch** out) {
  MultiDevice& m = *h->multi;
  auto it = m.xch.find(p);
  if (it != m.xch.end()) { *out = &it->second; return FMMBEM_OK; }
  const int W = m.world();
  MultiDevice::Xch x;
  x.send.assign(W, nullptr); x.recv.assign(W, nullptr); x.sc.resize(W); x.rc.resize(W);
  int prev = 0;
  (void)hipGetDevice(&prev);
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{prev};
  for (int r = 0; r < W; ++r) {
    x.sc[r].assign(W, 0); x.rc[r].assign(W, 0);
    TRY(fmmbem_plan_exchange_counts(m.shards[r].get(), p, x.sc[r].data(), x.rc[r].data()));
    int64_t ns = 0, nr = 0;
    for (int q = 0; q < W; ++q) { ns += x.sc[r][q]; nr += x.rc[r][q]; }
    HIP_TRY(hipSetDevice(m.dev[r]));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&x.send[r]), sizeof(double) * (size_t)std::max<int64_t>(ns, 1)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&x.recv[r]), sizeof(double) * (size_t)std::max<int64_t>(nr, 1)));
  }
  for (int r = 0; r < W; ++r)                          // what r sends q is what q expects from r, or the lists are broken
    for (int q = 0; q < W; ++q)
      if (x.sc[r][q] != x.rc[q][r]) return fail(FMMBEM_ERR_INVALID, "internal: exchange counts of the shards do not match");
  *out = &m.xch.emplace(p, std::move(x)).first->second;
  return FMMBEM_OK;
}

static int multi_execute_device(fmmbem_plan* h, int p, const double* d_x, double* d_y, hipStream_t s0) {
  MultiDevice& m = *h->multi;
  const int W = m.world();
  if (!d_x || !d_y) return fail(FMMBEM_ERR_INVALID, "null vector");
  const size_t nd = (size_t)h->hp.n * h->d.dof;
  int prev = 0;
  (void)hipGetDevice(&prev);
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{prev};
  MultiDevice::Xch* xc = nullptr;
  if (m.split) TRY(multi_xch(h, p, &xc));
  HIP_TRY(hipSetDevice(m.dev[0]));
  HIP_TRY(hipEventRecord(m.ev_x, s0));
  // Every device's share of a phase is ISSUED by a thread of its own (host_parallel): one thread took 0.43 ms to issue a matvec
  // over eight devices -- as long as a shard's share of the work runs (FMMBEM_MULTI_ISSUE_THREADS=0: the one thread).  A phase's
  // events are all recorded when its fan-out returns, which is what the next phase waits on.
  const bool threads = W > 1 && sw::multi_issue_threads();
  std::vector<int> rcs((size_t)W, FMMBEM_OK);
  std::vector<std::string> errs((size_t)W);
  auto fan_out = [&](auto&& body) -> int {
    auto one = [&](int r) {
      rcs[(size_t)r] = body(r);
      if (rcs[(size_t)r] != FMMBEM_OK) errs[(size_t)r] = fmmbem_last_error();     // (the text is the issuing thread's own)
    };
    if (threads) host_parallel(W, one); else for (int r = 0; r < W; ++r) one(r);
    for (int r = 0; r < W; ++r) if (rcs[(size_t)r] != FMMBEM_OK) return fail(rcs[(size_t)r], errs[(size_t)r]);
    return FMMBEM_OK;
  };
  TRY(fan_out([&](int r) -> int {                      // x to every device; the owners' upward pass
    fmmbem_plan& sh = *m.shards[r];
    HIP_TRY(hipSetDevice(m.dev[r]));
    HIP_TRY(hipStreamWaitEvent(sh.own_stream, m.ev_x, 0));
    HIP_TRY(hipMemcpyPeerAsync(m.x[r], m.dev[r], d_x, m.dev[0], sizeof(double) * nd, sh.own_stream));
    if (m.split) {
      TRY(sh.run(p, m.x[r], nullptr, sh.own_stream, false, fmmbem_plan::Phase::Upward, xc->send[r]));
      HIP_TRY(hipEventRecord(m.ev_up[r], sh.own_stream));
    }
    return FMMBEM_OK;
  }));
  // (the waits on the other shards' events in a fan-out of their own: a shard whose downward pass is being CAPTURED into a graph
  // on one thread makes another thread's wait on an event of that stream fail -- "dependency created on uncaptured work")
  if (m.split)
    TRY(fan_out([&](int q) -> int {                    // the multipoles q's lists read
      fmmbem_plan& sh = *m.shards[q];
      HIP_TRY(hipSetDevice(m.dev[q]));
      int64_t roff = 0;
      for (int r = 0; r < W; ++r) {
        const int64_t cnt = xc->rc[q][r];
        if (cnt > 0) {
          int64_t soff = 0;
          for (int k = 0; k < q; ++k) soff += xc->sc[r][k];
          HIP_TRY(hipStreamWaitEvent(sh.own_stream, m.ev_up[r], 0));
          HIP_TRY(hipMemcpyPeerAsync(xc->recv[q] + roff, m.dev[q], xc->send[r] + soff, m.dev[r], sizeof(double) * (size_t)cnt, sh.own_stream));
        }
        roff += cnt;
      }
      return FMMBEM_OK;
    }));
  TRY(fan_out([&](int q) -> int {                      // q's downward pass and near field, its slice home
    fmmbem_plan& sh = *m.shards[q];
    HIP_TRY(hipSetDevice(m.dev[q]));
    if (m.split) TRY(sh.run(p, nullptr, m.slice[q], sh.own_stream, false, fmmbem_plan::Phase::Downward, xc->recv[q]));
    else TRY(sh.run(p, m.x[q], m.slice[q], sh.own_stream, false));
    const size_t rows = (size_t)(m.cut[q + 1] - m.cut[q]) * h->d.dof;
    if (rows) HIP_TRY(hipMemcpyPeerAsync(m.gathered + (size_t)q * m.chunk, m.dev[0], m.slice[q], m.dev[q], sizeof(double) * rows, sh.own_stream));
    HIP_TRY(hipEventRecord(m.ev_done[q], sh.own_stream));
    return FMMBEM_OK;
  }));
  HIP_TRY(hipSetDevice(m.dev[0]));
  for (int q = 0; q < W; ++q) HIP_TRY(hipStreamWaitEvent(s0, m.ev_done[q], 0));
  TRY(fmmbem_plan_assemble_slices_device(m.shards[0].get(), m.gathered, m.chunk, d_y, s0));
  h->last_p = p;
  return FMMBEM_OK;
}

int fmmbem_plan_create(const fmmbem_options* opts, size_t n_panels, const double* vertices, const uint8_t* bc,
                       fmmbem_plan** out) {
  if (!opts || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  *out = nullptr;
  if (opts->kernel != FMMBEM_KERNEL_LAPLACE_BEM && opts->kernel != FMMBEM_KERNEL_STOKES_BEM)
    return fail(FMMBEM_ERR_UNSUPPORTED, "unknown kernel id");
  if (opts->kernel == FMMBEM_KERNEL_STOKES_BEM) {
    if (!(opts->mu > 0)) return fail(FMMBEM_ERR_INVALID, "Stokes: viscosity mu must be positive");
    // TRACTION panels: the near blocks are eval_traction_integral (kernel/StokesSphericalBEM.hpp:160-258).  Their far field
    // is the double-layer decomposition of kernels_far.hip (seven dipole potentials), checked against the Direct sum -- the
    // reference's own far field for this operator disagrees with its Direct sum by 50-75 %, so there
    // is nothing of the reference's to be equal to beyond Direct.  Orders up to 12 take the rotation M2L kernel, 13 ... 16 the
    // double sum over the eleven slots, one slot per pass.
  }
  if (!vertices || n_panels == 0) return fail(FMMBEM_ERR_INVALID, "no panels");
  if (opts->l2l_rule != FMMBEM_L2L_COMPLETE && opts->l2l_rule != FMMBEM_L2L_REFERENCE) return fail(FMMBEM_ERR_INVALID, "unknown l2l_rule");
  const bool tree = opts->evaluator == FMMBEM_EVAL_TREECODE;
  if (!tree && (opts->evaluator < FMMBEM_EVAL_FMM || opts->evaluator > FMMBEM_EVAL_BLOCK_DIAGONAL)) return fail(FMMBEM_ERR_INVALID, "unknown evaluator");
  if (opts->near_f32_max_p < 0 || opts->near_f32_max_p > 16) return fail(FMMBEM_ERR_INVALID, "near_f32_max_p outside 0..16");
  if (opts->stokes_batch_width < 0 || opts->stokes_batch_width > 4) return fail(FMMBEM_ERR_INVALID, "stokes_batch_width outside 0..4");
  // The treecode evaluator: M2P is built for the Laplace kernel, on one device, whole operator.  The hybrid and the float near
  // field are taken as off (the options as the plan and the geometry cache then see them)
  fmmbem_options tree_opts;
  if (tree) {
    if (opts->kernel == FMMBEM_KERNEL_STOKES_BEM) return fail(FMMBEM_ERR_UNSUPPORTED, "treecode evaluator: Laplace only (the Stokes M2P is not built)");
    if (opts->shard_world > 1) return fail(FMMBEM_ERR_UNSUPPORTED, "treecode evaluator: shard_world > 1 is not built");
    if (opts->n_devices > 1 || (opts->n_devices == 0 && !opts->host_only && !sw::devices().empty()))
      return fail(FMMBEM_ERR_UNSUPPORTED, "treecode evaluator: a device list (n_devices > 1 or FMMBEM_DEVICES) is not built");
    tree_opts = *opts;
    tree_opts.near_stream_fraction = 1.0;
    tree_opts.near_f32_max_p = 0;
    opts = &tree_opts;
  }
  // The geometry of a live plan, recognised: same options, same panel count, same vertex bytes (two 64-bit hashes) -- only the
  // boundary-condition flags may differ.  The new plan then shares that plan's tree, lists and tables (PlanShared) and builds
  // only what the flags decide.  This is the drivers' second plan (examples/LaplaceBEM.cpp:218-232: the same panels with the
  // flags switched, for the right-hand side); FMMBEM_PLAN_SHARE=0 turns the recognition off.
  {
    // a device list: the options' own, or FMMBEM_DEVICES=0,1,2,... for callers that cannot say (the reference's unmodified drivers)
    std::vector<int> devices;
    if (opts->n_devices > 1) devices.assign(opts->devices, opts->devices + std::min(opts->n_devices, 8));
    else if (opts->n_devices == 0 && opts->shard_world <= 1 && !opts->host_only) devices = sw::devices();
    if (!devices.empty()) {
      if (opts->host_only) return fail(FMMBEM_ERR_INVALID, "a device list and host_only exclude each other");
      return multi_create(opts, devices, n_panels, vertices, bc, out);
    }
  }
  if (!opts->host_only) (void)order_tables();             // the order tables start building now, beside the tree
  uint64_t fp[2] = {0, 0};
  const bool share_on = !opts->host_only && sw::plan_share();
  if (share_on) {
    fingerprint_vertices(vertices, n_panels, fp);
    if (std::shared_ptr<PlanShared> sh = geometry_cache_find(n_panels, fp, *opts)) {
      fmmbem_options o = sh->geo.opts;
      o.stokes_batch_width = opts->stokes_batch_width;              // no part of the geometry: the new plan's own
      return fmmbem_plan::like(std::move(sh), o, bc, out);
    }
  }
  std::unique_ptr<fmmbem_plan> pl(new (std::nothrow) fmmbem_plan(std::make_shared<PlanShared>()));
  if (!pl) return fail(FMMBEM_ERR_ALLOC, "plan");
  PlanGeometry& geo = pl->shared->geo;                  // written here and by to_device_near / to_device_far, then never again
  pl->opts = geo.opts = *opts;
  pl->shared->fingerprint[0] = fp[0]; pl->shared->fingerprint[1] = fp[1];
  HostOptions ho;
  ho.p_max = opts->p_max; ho.quad_k = opts->quad_k; ho.theta = opts->theta; ho.ncrit = opts->ncrit;
  ho.shard_rank = opts->shard_rank; ho.shard_world = opts->shard_world < 1 ? 1 : opts->shard_world;
  ho.evaluator = tree ? (int)FMMBEM_EVAL_FMM : opts->evaluator;   // a treecode plan's tree and lists ARE the FMM plan's
  ho.shard_upward = opts->shard_upward < 0 ? 0 : opts->shard_upward > 2 ? 2 : opts->shard_upward;
  ho.reference_l2l = opts->l2l_rule == FMMBEM_L2L_REFERENCE;
  ho.panels_on_device = !opts->host_only && !sw::panels_on_host();
  const double t0 = now_ms();
  // The near field goes to the device as soon as the host plan holds what it needs -- the panels' geometry, the leaves, the
  // near lists -- and its assembly runs on the GPU while the host builds the far-field lists (FMMBEM_BUILD_TWO_PHASE=0: after them)
  int near_rc = FMMBEM_OK;
  bool near_done = false;
  double near_ms = 0;
  if (!opts->host_only && ho.panels_on_device && sw::build_two_phase())
    ho.after_near_lists = [&]() -> std::string {
      const double t = now_ms();
      pl->has_bc[0] = pl->hp.has_bc[0]; pl->has_bc[1] = pl->hp.has_bc[1];
      pl->create_vertices = vertices;
      try {
        near_rc = pl->to_device_near(geo);
      } catch (const std::bad_alloc&) {
        near_rc = fail(FMMBEM_ERR_ALLOC, "host allocation failed while tabulating operators");
      }
      pl->create_vertices = nullptr;
      near_done = true;
      near_ms = now_ms() - t;
      return near_rc == FMMBEM_OK ? std::string() : std::string("device");
    };
  std::string err;
  try {
    err = pl->hp.build(ho, (int64_t)n_panels, vertices, bc);
  } catch (const std::bad_alloc&) {
    return fail(FMMBEM_ERR_ALLOC, "host allocation failed while building the plan");
  }
  pl->hp.opt.after_near_lists = nullptr;                // (it refers to this frame)
  if (near_rc != FMMBEM_OK) return near_rc;
  if (!err.empty()) return fail(err.find("octree") != std::string::npos ? FMMBEM_ERR_TREE : FMMBEM_ERR_INVALID, err);
  pl->build_host_ms = now_ms() - t0 - near_ms;
  pl->has_bc[0] = pl->hp.has_bc[0]; pl->has_bc[1] = pl->hp.has_bc[1];
  if (!opts->host_only) {
    try {
      pl->create_vertices = ho.panels_on_device ? vertices : nullptr;
      int rc = near_done ? FMMBEM_OK : pl->to_device_near(geo);
      pl->create_vertices = nullptr;
      if (rc == FMMBEM_OK) rc = pl->to_device_far(geo);
      if (rc != FMMBEM_OK) return rc;
    } catch (const std::bad_alloc&) {
      return fail(FMMBEM_ERR_ALLOC, "host allocation failed while tabulating operators");
    }
    // vertices are only needed on the device; keep the host copy small
    pl->hp.panels.vert.clear(); pl->hp.panels.vert.shrink_to_fit();
    if (share_on) geometry_cache_add(pl->shared);
  }
  *out = pl.release();
  return FMMBEM_OK;
}

// ---- plans over separate targets (include/fmmbem.h fmmbem_plan_create_targets) ----
// FMM_plan(K, sources, targets, opts) of the reference (include/FMM_plan.hpp:45-55): y_i = sum_j K(t_i, s_j) x_j at target POINTS,
// the target's flag picking G or dG/dn.  One host plan over both trees (HostPlan::build_targets), then the single plan's device
// path: the near rows are the target points (the same entry functions, so a target on a panel's centroid gets that row's bits),
// the far field runs P2M/M2M on the source boxes, M2L from source to target boxes, L2L/L2P on the target boxes.
static int target_plan_only(const fmmbem_plan* plan, const char* what) {
  if (plan && plan->targets)
    return fail(FMMBEM_ERR_UNSUPPORTED, std::string(what) + ": not on a plan over separate targets (fmmbem_plan_create_targets)");
  return FMMBEM_OK;
}

// The one builder of dual plans.  field: fmmbem_plan_create_field, which takes the Stokes kernel too (dof = 3: the single Stokes
// plan's near blocks, P2M, tree passes and L2P on the two trees); the four-argument form of the reference keeps refusing it.
static int create_dual(bool field, const fmmbem_options* opts, size_t n_panels, const double* vertices,
                       size_t n_targets, const double* target_points, const uint8_t* target_bc, fmmbem_plan** out) {
  if (!opts || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!vertices || n_panels == 0) return fail(FMMBEM_ERR_INVALID, "no panels");
  if (!target_points || n_targets == 0) return fail(FMMBEM_ERR_INVALID, "no targets");
  if (opts->near_f32_max_p < 0 || opts->near_f32_max_p > 16) return fail(FMMBEM_ERR_INVALID, "near_f32_max_p outside 0..16");
  if (opts->stokes_batch_width < 0 || opts->stokes_batch_width > 4) return fail(FMMBEM_ERR_INVALID, "stokes_batch_width outside 0..4");
  if (opts->kernel == FMMBEM_KERNEL_STOKES_BEM) {
    if (!field) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: Laplace only (the Stokes field at points: fmmbem_plan_create_field)");
    if (!(opts->mu > 0)) return fail(FMMBEM_ERR_INVALID, "Stokes: viscosity mu must be positive");
  } else if (opts->kernel != FMMBEM_KERNEL_LAPLACE_BEM) return fail(FMMBEM_ERR_UNSUPPORTED, "unknown kernel id");
  if (opts->shard_world > 1) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: shard_world > 1 is not implemented");
  if (opts->n_devices > 1) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: a device list is not implemented");
  if (opts->evaluator != FMMBEM_EVAL_FMM) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: the FMM evaluator only");
  if (!opts->sparse_local) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: the assembled near field only (sparse_local = 1)");
  if (opts->l2l_rule != FMMBEM_L2L_COMPLETE) return fail(FMMBEM_ERR_UNSUPPORTED, "target plans: l2l_rule COMPLETE only");
  if (n_panels + n_targets > (size_t)INT32_MAX) return fail(FMMBEM_ERR_INVALID, "too many panels and targets");
  if (!opts->host_only) (void)order_tables();
  std::unique_ptr<fmmbem_plan> pl(new (std::nothrow) fmmbem_plan(std::make_shared<PlanShared>()));
  if (!pl) return fail(FMMBEM_ERR_ALLOC, "plan");
  PlanGeometry& geo = pl->shared->geo;
  pl->opts = *opts;
  pl->opts.near_stream_fraction = 1.0;                 // the hybrid near field is taken as 1 here
  pl->opts.near_f32_max_p = 0;                         // ... and the float near field as off
  pl->opts.shard_rank = 0; pl->opts.shard_world = 1; pl->opts.n_devices = 0;
  geo.opts = pl->opts;
  pl->targets = true;
  HostOptions ho;
  ho.p_max = opts->p_max; ho.quad_k = opts->quad_k; ho.theta = opts->theta; ho.ncrit = opts->ncrit;
  const double t0 = now_ms();
  std::string err;
  try {
    err = pl->hp.build_targets(ho, (int64_t)n_panels, vertices, (int64_t)n_targets, target_points, target_bc);
  } catch (const std::bad_alloc&) {
    return fail(FMMBEM_ERR_ALLOC, "host allocation failed while building the plan");
  }
  if (!err.empty()) return fail(err.find("octree") != std::string::npos ? FMMBEM_ERR_TREE : FMMBEM_ERR_INVALID, err);
  pl->build_host_ms = now_ms() - t0;
  pl->has_bc[0] = pl->hp.has_bc[0]; pl->has_bc[1] = pl->hp.has_bc[1];
  if (!opts->host_only) {
    try {
      TRY(pl->to_device_near(geo));
      TRY(pl->to_device_far(geo));
      DEVICE_SCOPE(opts->device);
      const HostPlan& h = pl->hp;
      for (int l = h.leaf_begin; l < h.leaf_end; ++l) pl->zero_target_rows = pl->zero_target_rows || h.near_ncols[l] == 0;
      bool coincide = false;
      for (size_t k = 0; k < h.target_point.size() && !coincide; ++k) coincide = h.target_point[k] != (uint32_t)k;
      const size_t dof = (size_t)geo.gd.dof;
      if (coincide) {
        TRY(pl->upload(h.target_point, &pl->d_target_point));
        TRY(pl->alloc((size_t)(h.n - h.n_src) * dof, &pl->y_points, true));
      }
      TRY(pl->alloc((size_t)n_targets * dof, &pl->stage_y_targets, true));
      HIP_TRY(hipDeviceSynchronize());
    } catch (const std::bad_alloc&) {
      return fail(FMMBEM_ERR_ALLOC, "host allocation failed while tabulating operators");
    }
    pl->hp.panels.vert.clear(); pl->hp.panels.vert.shrink_to_fit();
  }
  *out = pl.release();
  return FMMBEM_OK;
}

int fmmbem_plan_create_targets(const fmmbem_options* opts, size_t n_panels, const double* vertices, const uint8_t* bc,
                               size_t n_targets, const double* target_points, const uint8_t* target_bc, fmmbem_plan** out) {
  (void)bc;       // the sources' flags do not enter: the target's flag picks the kernel (kernel/LaplaceSphericalBEM.hpp:273-297)
  return create_dual(false, opts, n_panels, vertices, n_targets, target_points, target_bc, out);
}

int fmmbem_plan_create_field(const fmmbem_options* opts, size_t n_panels, const double* vertices,
                             size_t n_targets, const double* target_points, const uint8_t* target_bc, fmmbem_plan** out) {
  return create_dual(true, opts, n_panels, vertices, n_targets, target_points, target_bc, out);
}

int fmmbem_plan_target_info(const fmmbem_plan* plan, fmmbem_target_info* o) {
  if (!plan || !o) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (!plan->targets) return fail(FMMBEM_ERR_INVALID, "not a plan over separate targets");
  const HostPlan& h = plan->hp;
  std::memset(o, 0, sizeof(*o));
  o->n_panels = h.n_src;
  o->n_targets = h.n_targets;
  o->n_target_points = h.n - h.n_src;
  o->n_source_boxes = (int64_t)h.src_box.size(); o->n_source_leaves = h.src_nleaves; o->n_source_levels = h.src_nlevels;
  o->n_target_boxes = (int64_t)h.tgt_box.size(); o->n_target_leaves = h.tgt_nleaves; o->n_target_levels = h.tgt_nlevels;
  o->tree_coder_levels = h.tree_levels_max;
  return FMMBEM_OK;
}

// the boxes of one tree of a dual plan, in that tree's own BFS numbering; bodies counted from 0 in that tree
static void dual_boxes(const HostPlan& h, bool tgt, double* center, double* side, int32_t* level, int32_t* is_leaf, int32_t* parent,
                       int32_t* body_begin, int32_t* body_end) {
  const std::vector<int>& map = tgt ? h.tgt_box : h.src_box;
  std::vector<int> local((size_t)h.nboxes, -1);
  for (size_t b = 0; b < map.size(); ++b) local[(size_t)map[b]] = (int)b;
  const int64_t body0 = tgt ? h.n_src : 0;
  for (size_t b = 0; b < map.size(); ++b) {
    const int u = map[b];
    if (center) std::memcpy(center + 3 * b, &h.box_center[3 * (size_t)u], sizeof(double) * 3);
    if (side) side[b] = h.box_side[u];
    if (level) level[b] = h.box_level[u];
    if (is_leaf) is_leaf[b] = h.box_leaf[u];
    if (parent) parent[b] = b == 0 ? 0 : local[(size_t)h.box_parent[u]];
    if (body_begin) body_begin[b] = (int32_t)(h.box_body_begin[u] - body0);
    if (body_end) body_end[b] = (int32_t)(h.box_body_end[u] - body0);
  }
}

int fmmbem_plan_get_target_boxes(const fmmbem_plan* plan, double* center, double* side, int32_t* level, int32_t* is_leaf,
                                 int32_t* parent, int32_t* body_begin, int32_t* body_end) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (!plan->targets) return fail(FMMBEM_ERR_INVALID, "not a plan over separate targets");
  dual_boxes(plan->hp, true, center, side, level, is_leaf, parent, body_begin, body_end);
  return FMMBEM_OK;
}

int fmmbem_plan_get_target_perm(const fmmbem_plan* plan, uint32_t* tree_to_point, uint32_t* target_to_point) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (!plan->targets) return fail(FMMBEM_ERR_INVALID, "not a plan over separate targets");
  const HostPlan& h = plan->hp;
  if (tree_to_point) std::memcpy(tree_to_point, h.perm.data() + h.n_src, sizeof(uint32_t) * (size_t)(h.n - h.n_src));
  if (target_to_point) std::memcpy(target_to_point, h.target_point.data(), sizeof(uint32_t) * h.target_point.size());
  return FMMBEM_OK;
}

int fmmbem_plan_create_like(const fmmbem_plan* base, const uint8_t* bc, fmmbem_plan** out) {
  if (!base || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  *out = nullptr;
  TRY(target_plan_only(base, "fmmbem_plan_create_like"));
  if (!base->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "fmmbem_plan_create_like: the base plan was built host-only");
  if (base->multi) return multi_like(*base, bc, out);
  return fmmbem_plan::like(base->shared, base->opts, bc, out);
}

void fmmbem_plan_destroy(fmmbem_plan* plan) { delete plan; }

int fmmbem_plan_execute_device(fmmbem_plan* plan, int p, const double* d_x, double* d_y, void* stream) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (plan->multi) return multi_execute_device(plan, p, d_x, d_y, static_cast<hipStream_t>(stream));
  return plan->run(p, d_x, d_y, static_cast<hipStream_t>(stream), false);
}

static int single_device_only(const fmmbem_plan* plan) {
  return plan && plan->multi ? fail(FMMBEM_ERR_UNSUPPORTED, "not on a multi-device plan: it drives its shards itself") : FMMBEM_OK;
}
// The guard of the shard and split entry points: refuses a target plan, then the handle of a multi-device plan, then a null plan
// (fmmbem_plan_exchange_doubles looks at its arguments before the multi-device check: it spells its own order with the pieces)
static int shard_entry(const fmmbem_plan* plan, const char* what, const char* if_null = "null plan") {
  TRY(target_plan_only(plan, what));
  TRY(single_device_only(plan));
  return plan ? FMMBEM_OK : fail(FMMBEM_ERR_INVALID, if_null);
}

// expansion slots an exchange carries per box, from the HOST lists (a host-only plan answers too): Laplace one per boundary
// condition present; Stokes four potentials for velocity targets, seven for TRACTION targets (to_device, d.act)
static int64_t active_slots(const fmmbem_plan* plan) {
  const HostPlan& h = plan->hp;
  if (plan->opts.kernel != FMMBEM_KERNEL_STOKES_BEM) return (int64_t)plan->has_bc[0] + (int64_t)plan->has_bc[1];
  const bool trac = plan->has_bc[1] && h.opt.evaluator == 0;
  const bool vel = plan->has_bc[0] || !trac;
  return (vel ? 4 : 0) + (trac ? 7 : 0);
}

int fmmbem_plan_exchange_doubles(const fmmbem_plan* plan, int p, size_t* per_shard) {
  TRY(target_plan_only(plan, "fmmbem_plan_exchange_doubles"));
  if (!plan || !per_shard) return fail(FMMBEM_ERR_INVALID, "null argument");
  TRY(single_device_only(plan));
  if (p < 1 || p > plan->hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  // from the host lists, so that a host-only plan (CPU tests of the N > 1 path) answers too
  const HostPlan& h = plan->hp;
  size_t most = 0;
  for (size_t r = 0; r + 1 < h.xch_ptr.size(); ++r) most = std::max<size_t>(most, (size_t)(h.xch_ptr[r + 1] - h.xch_ptr[r]));
  const size_t n_act = (size_t)active_slots(plan);
  *per_shard = (h.opt.shard_upward && h.opt.shard_world > 1) ? most * n_act * (size_t)(p * (p + 1) / 2) * 2 : 0;
  return FMMBEM_OK;
}

int fmmbem_plan_exchange_counts(const fmmbem_plan* plan, int p, int64_t* send_doubles, int64_t* recv_doubles) {
  TRY(shard_entry(plan, "fmmbem_plan_exchange_counts", "null argument"));
  if (!send_doubles || !recv_doubles) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (p < 1 || p > plan->hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  const HostPlan& h = plan->hp;
  const int W = h.opt.shard_world;
  const bool sel = h.opt.shard_upward == 2 && W > 1;
  if (!sel) return fail(FMMBEM_ERR_INVALID, "plan was not created with shard_upward = 2");
  const int64_t n_act = active_slots(plan);
  const int64_t per = n_act * (int64_t)(p * (p + 1) / 2) * 2;
  for (int q = 0; q < W; ++q) {
    send_doubles[q] = (int64_t)(h.xsel_send_ptr[q + 1] - h.xsel_send_ptr[q]) * per;
    recv_doubles[q] = (int64_t)(h.xsel_recv_ptr[q + 1] - h.xsel_recv_ptr[q]) * per;
  }
  return FMMBEM_OK;
}

int fmmbem_plan_upward_device(fmmbem_plan* plan, int p, const double* d_x, double* d_send, void* stream) {
  TRY(shard_entry(plan, "fmmbem_plan_upward_device"));
  return plan->run(p, d_x, nullptr, static_cast<hipStream_t>(stream), false, fmmbem_plan::Phase::Upward, d_send);
}

int fmmbem_plan_downward_device(fmmbem_plan* plan, int p, const double* d_recv, double* d_y, void* stream) {
  TRY(shard_entry(plan, "fmmbem_plan_downward_device"));
  return plan->run(p, nullptr, d_y, static_cast<hipStream_t>(stream), false, fmmbem_plan::Phase::Downward, const_cast<double*>(d_recv));
}

int fmmbem_plan_near_split_device(fmmbem_plan* plan, double* d_y, void* stream) {
  TRY(shard_entry(plan, "fmmbem_plan_near_split_device"));
  return plan->run(plan->last_p > 0 ? plan->last_p : 1, nullptr, d_y, static_cast<hipStream_t>(stream), false, fmmbem_plan::Phase::NearSplit, nullptr);
}

int fmmbem_plan_shard_rows(const fmmbem_plan* plan, int64_t* cut) {
  TRY(target_plan_only(plan, "fmmbem_plan_shard_rows"));
  if (!plan || !cut) return fail(FMMBEM_ERR_INVALID, "null argument");
  const HostPlan& h = plan->hp;
  std::vector<int> leaf_cut;
  partition_leaves(h, h.opt.shard_world, leaf_cut);
  for (int r = 0; r <= h.opt.shard_world; ++r)
    cut[r] = leaf_cut[r] < h.nleaves() ? (int64_t)h.box_body_begin[h.leaf_box[leaf_cut[r]]] : h.n;
  return FMMBEM_OK;
}

int fmmbem_plan_set_result_slices(fmmbem_plan* plan, int enabled) {
  TRY(shard_entry(plan, "fmmbem_plan_set_result_slices"));
  plan->result_slices = enabled != 0;
  return FMMBEM_OK;
}

int fmmbem_plan_assemble_slices_device(fmmbem_plan* plan, const double* d_slices, size_t chunk_doubles, double* d_y, void* stream) {
  TRY(target_plan_only(plan, "fmmbem_plan_assemble_slices_device"));
  if (!plan || !d_slices || !d_y) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "plan was built host-only; there is no CPU execution path");
  const int world = plan->hp.opt.shard_world;
  DEVICE_SCOPE(plan->opts.device);
  if (!plan->d_cut) {
    std::vector<int64_t> cut((size_t)world + 1);
    TRY(fmmbem_plan_shard_rows(plan, cut.data()));
    for (int r = 0; r < world; ++r)
      if ((size_t)(cut[r + 1] - cut[r]) * plan->d.dof > chunk_doubles) return fail(FMMBEM_ERR_INVALID, "chunk smaller than a shard's slice");
    TRY(plan->alloc((size_t)world + 1, &plan->d_cut, false));
    HIP_TRY(hipMemcpy(plan->d_cut, cut.data(), sizeof(int64_t) * cut.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_assemble_slices(plan->d, d_slices, d_y, world, plan->d_cut, (int64_t)chunk_doubles, static_cast<hipStream_t>(stream)));
  return FMMBEM_OK;
}

int fmmbem_plan_near_device(fmmbem_plan* plan, const double* d_x, double* d_y, void* stream) {
  TRY(single_device_only(plan));
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  return plan->run(1, d_x, d_y, static_cast<hipStream_t>(stream), true);
}

int fmmbem_plan_execute(fmmbem_plan* plan, int p, const double* x, double* y) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (!plan->on_device && plan->targets) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "plan was built host-only; there is no CPU execution path");
  if (!x || !y) return fail(FMMBEM_ERR_INVALID, "null vector");
  if (plan->result_slices)         // the owned rows in tree order at the head of y are only meaningful to the device-side all-gather
    return fail(FMMBEM_ERR_INVALID, "plan delivers result slices (fmmbem_plan_set_result_slices): use the device entry points");
  DEVICE_SCOPE(plan->opts.device);
  const size_t bytes_x = sizeof(double) * plan->x_doubles(), bytes_y = sizeof(double) * plan->y_doubles();
  double* sy = plan->targets ? plan->stage_y_targets : plan->stage_y;
  hipStream_t s = plan->own_stream;
  HIP_TRY(hipMemcpyAsync(plan->stage_x, x, bytes_x, hipMemcpyHostToDevice, s));
  const int rc = plan->multi ? multi_execute_device(plan, p, plan->stage_x, sy, s) : plan->run(p, plan->stage_x, sy, s, false);
  if (rc != FMMBEM_OK) return rc;
  HIP_TRY(hipMemcpyAsync(y, sy, bytes_y, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FMMBEM_OK;
}

// ---- field quantities (include/fmmbem.h) ----
static int field_execute_device(fmmbem_plan* plan, FieldQuantity q, int p, const double* d_x, double* d_out, void* stream) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  return plan->run_field(q, p, d_x, d_out, static_cast<hipStream_t>(stream));
}

static int field_execute(fmmbem_plan* plan, FieldQuantity q, int p, const double* x, double* out) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (!x || !out) return fail(FMMBEM_ERR_INVALID, "null vector");
  TRY(plan->field_refusal(q, p));                      // a refusal touches neither pointer
  DEVICE_SCOPE(plan->opts.device);
  TRY(plan->field_alloc(q));
  double* stage = plan->field[(int)q].stage;
  hipStream_t s = plan->own_stream;
  HIP_TRY(hipMemcpyAsync(plan->stage_x, x, sizeof(double) * plan->x_doubles(), hipMemcpyHostToDevice, s));
  TRY(plan->run_field(q, p, plan->stage_x, stage, s));
  HIP_TRY(hipMemcpyAsync(out, stage, sizeof(double) * kField[(int)q].width * (size_t)plan->hp.n_targets, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FMMBEM_OK;
}

int fmmbem_plan_execute_gradient_device(fmmbem_plan* plan, int p, const double* d_x, double* d_g, void* stream) {
  return field_execute_device(plan, FieldQuantity::Gradient, p, d_x, d_g, stream);
}
int fmmbem_plan_execute_gradient(fmmbem_plan* plan, int p, const double* x, double* g) {
  return field_execute(plan, FieldQuantity::Gradient, p, x, g);
}
int fmmbem_plan_execute_hessian_device(fmmbem_plan* plan, int p, const double* d_x, double* d_H, void* stream) {
  return field_execute_device(plan, FieldQuantity::Hessian, p, d_x, d_H, stream);
}
int fmmbem_plan_execute_hessian(fmmbem_plan* plan, int p, const double* x, double* H) {
  return field_execute(plan, FieldQuantity::Hessian, p, x, H);
}
int fmmbem_plan_execute_pressure_device(fmmbem_plan* plan, int p, const double* d_x, double* d_q, void* stream) {
  return field_execute_device(plan, FieldQuantity::Pressure, p, d_x, d_q, stream);
}
int fmmbem_plan_execute_pressure(fmmbem_plan* plan, int p, const double* x, double* q) {
  return field_execute(plan, FieldQuantity::Pressure, p, x, q);
}
int fmmbem_plan_execute_velocity_gradient_device(fmmbem_plan* plan, int p, const double* d_x, double* d_G, void* stream) {
  return field_execute_device(plan, FieldQuantity::VelocityGradient, p, d_x, d_G, stream);
}
int fmmbem_plan_execute_velocity_gradient(fmmbem_plan* plan, int p, const double* x, double* G) {
  return field_execute(plan, FieldQuantity::VelocityGradient, p, x, G);
}

// ---- flow execute (include/fmmbem.h) ----
int fmmbem_plan_execute_flow_device(fmmbem_plan* plan, int p, const double* d_x, double* d_u, double* d_q, double* d_G, void* stream) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  return plan->run_flow(p, d_x, d_u, d_q, d_G, static_cast<hipStream_t>(stream));
}
int fmmbem_plan_execute_flow(fmmbem_plan* plan, int p, const double* x, double* u, double* q, double* G) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (!x || (!u && !q && !G)) return fail(FMMBEM_ERR_INVALID, "null vector, or no output asked");
  TRY(plan->flow_refusal(p));                          // a refusal touches no pointer
  DEVICE_SCOPE(plan->opts.device);
  if (q) TRY(plan->field_alloc(FieldQuantity::Pressure));
  if (G) TRY(plan->field_alloc(FieldQuantity::VelocityGradient));
  double* const sq = plan->field[(int)FieldQuantity::Pressure].stage;
  double* const sG = plan->field[(int)FieldQuantity::VelocityGradient].stage;
  const size_t nt = (size_t)plan->hp.n_targets;
  hipStream_t s = plan->own_stream;
  HIP_TRY(hipMemcpyAsync(plan->stage_x, x, sizeof(double) * plan->x_doubles(), hipMemcpyHostToDevice, s));
  TRY(plan->run_flow(p, plan->stage_x, u ? plan->stage_y_targets : nullptr, q ? sq : nullptr, G ? sG : nullptr, s));
  if (u) HIP_TRY(hipMemcpyAsync(u, plan->stage_y_targets, sizeof(double) * plan->y_doubles(), hipMemcpyDeviceToHost, s));
  if (q) HIP_TRY(hipMemcpyAsync(q, sq, sizeof(double) * nt, hipMemcpyDeviceToHost, s));
  if (G) HIP_TRY(hipMemcpyAsync(G, sG, sizeof(double) * 9 * nt, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FMMBEM_OK;
}

// ---- representation execute (include/fmmbem.h) ----
int fmmbem_plan_execute_representation_device(fmmbem_plan* plan, int p, const double* d_density, const double* d_potential, double* d_phi,
                                              double* d_grad, void* stream) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  return plan->run_representation(p, d_density, d_potential, d_phi, d_grad, static_cast<hipStream_t>(stream));
}
int fmmbem_plan_execute_representation(fmmbem_plan* plan, int p, const double* density, const double* potential, double* phi, double* grad) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if ((!density && !potential) || (!phi && !grad)) return fail(FMMBEM_ERR_INVALID, "no layer given, or no output asked");
  TRY(plan->representation_refusal(p));                // a refusal touches no pointer
  DEVICE_SCOPE(plan->opts.device);
  TRY(plan->representation_alloc(phi != nullptr, grad != nullptr));
  double* const sg = plan->field[(int)FieldQuantity::Gradient].stage;
  const size_t nt = (size_t)plan->hp.n_targets, bytes_x = sizeof(double) * plan->x_doubles();
  hipStream_t s = plan->own_stream;
  if (density) HIP_TRY(hipMemcpyAsync(plan->stage_x, density, bytes_x, hipMemcpyHostToDevice, s));
  if (potential) HIP_TRY(hipMemcpyAsync(plan->rep.stage_mu, potential, bytes_x, hipMemcpyHostToDevice, s));
  TRY(plan->run_representation(p, density ? plan->stage_x : nullptr, potential ? plan->rep.stage_mu : nullptr, phi ? plan->rep.phi_stage : nullptr,
                               grad ? sg : nullptr, s));
  if (phi) HIP_TRY(hipMemcpyAsync(phi, plan->rep.phi_stage, sizeof(double) * nt, hipMemcpyDeviceToHost, s));
  if (grad) HIP_TRY(hipMemcpyAsync(grad, sg, sizeof(double) * 3 * nt, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FMMBEM_OK;
}

// ---- batched execute (include/fmmbem.h) ----
static int batch_args(const fmmbem_plan* plan, int k, const void* x, size_t ldx, const void* y, size_t ldy) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (k < 1) return fail(FMMBEM_ERR_INVALID, "batch of k < 1 vectors");
  if (!x || !y) return fail(FMMBEM_ERR_INVALID, "null vector");
  if (ldx < plan->x_doubles() || ldy < plan->y_doubles()) return fail(FMMBEM_ERR_INVALID, "leading dimension shorter than a vector");
  return FMMBEM_OK;
}

// batches never capture or replay graphs: off for the call (on the shards of a device list too), restored after
struct GraphsOff {
  fmmbem_plan* pl;
  bool own;
  std::vector<bool> shard;
  explicit GraphsOff(fmmbem_plan* p) : pl(p), own(p->use_graphs) {
    pl->use_graphs = false;
    if (pl->multi) for (auto& sh : pl->multi->shards) { shard.push_back(sh->use_graphs); sh->use_graphs = false; }
  }
  ~GraphsOff() {
    pl->use_graphs = own;
    if (pl->multi) for (size_t r = 0; r < shard.size(); ++r) pl->multi->shards[r]->use_graphs = shard[r];
  }
};

static int batch_execute(fmmbem_plan* plan, int p, int k, const double* x, size_t ldx, double* y, size_t ldy, hipStream_t s, bool host) {
  GraphsOff off(plan);
  if (plan->batch_width() > 1) return plan->run_batch(p, k, x, ldx, y, ldy, s, host);
  for (int j = 0; j < k; ++j) {                        // vector by vector: exactly the single entry points
    const double* xj = x + (size_t)j * ldx;
    double* yj = y + (size_t)j * ldy;
    TRY(host ? fmmbem_plan_execute(plan, p, xj, yj) : fmmbem_plan_execute_device(plan, p, xj, yj, s));
  }
  return FMMBEM_OK;
}

int fmmbem_plan_execute_batch(fmmbem_plan* plan, int p, int k, const double* x, size_t ldx, double* y, size_t ldy) {
  TRY(batch_args(plan, k, x, ldx, y, ldy));
  if (!plan->on_device && plan->targets) return fail(FMMBEM_ERR_UNSUPPORTED, "target plan built host-only: no execute");
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "plan was built host-only; there is no CPU execution path");
  if (plan->result_slices)
    return fail(FMMBEM_ERR_INVALID, "plan delivers result slices (fmmbem_plan_set_result_slices): use the device entry points");
  return batch_execute(plan, p, k, x, ldx, y, ldy, plan->own_stream, true);
}

int fmmbem_plan_execute_batch_device(fmmbem_plan* plan, int p, int k, const double* d_x, size_t ldx, double* d_y, size_t ldy, void* stream) {
  TRY(batch_args(plan, k, d_x, ldx, d_y, ldy));
  return batch_execute(plan, p, k, d_x, ldx, d_y, ldy, static_cast<hipStream_t>(stream), false);
}

int fmmbem_plan_batch_width(const fmmbem_plan* plan, int* width) {
  if (!plan || !width) return fail(FMMBEM_ERR_INVALID, "null argument");
  *width = plan->batch_width();
  return FMMBEM_OK;
}

// ---- exact block-Jacobi preconditioner: the leaf blocks of a BLOCK_DIAGONAL plan inverted on the device (include/fmmbem.h) ----
static_assert(kBlockInvMax == FMMBEM_BLOCK_INVERSE_MAX, "the header states the largest leaf the kernels serve");
int fmmbem_plan_block_inverse_build(fmmbem_plan* plan) {
  const char* who = "fmmbem_plan_block_inverse_build: ";
  if (!plan) return fail(FMMBEM_ERR_INVALID, std::string(who) + "null plan");
  if (plan->targets || plan->opts.evaluator != FMMBEM_EVAL_BLOCK_DIAGONAL)
    return fail(FMMBEM_ERR_INVALID, std::string(who) + "needs a plan created with evaluator BLOCK_DIAGONAL");
  if (!plan->opts.sparse_local) return fail(FMMBEM_ERR_UNSUPPORTED, std::string(who) + "a matrix-free plan holds no blocks to invert");
  if (plan->multi || plan->opts.n_devices > 1) return fail(FMMBEM_ERR_UNSUPPORTED, std::string(who) + "not on a plan over a device list");
  if (plan->hp.opt.shard_world > 1 || plan->opts.shard_world > 1) return fail(FMMBEM_ERR_UNSUPPORTED, std::string(who) + "not on a shard of an operator");
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, std::string(who) + "plan was built host-only; the blocks live on the device");
  if (plan->binv.built) return FMMBEM_OK;
  if (plan->g.hybrid || (!plan->d.near_val && !plan->d.near_sym)) return fail(FMMBEM_ERR_UNSUPPORTED, std::string(who) + "the plan stores no leaf blocks");
  const HostPlan& h = plan->hp;
  const int dof = plan->d.dof;
  // every leaf of a BLOCK_DIAGONAL plan is its own and only source (EvalDiagonalSparse.hpp:33-49)
  std::vector<int> selfcol((size_t)h.nleaves(), 0);
  std::vector<int64_t> off((size_t)(h.leaf_end - h.leaf_begin) + 1, 0);
  int max_m = 0;
  for (int l = h.leaf_begin; l < h.leaf_end; ++l) {
    if (h.near_ptr[l + 1] - h.near_ptr[l] != 1 || h.near_src[h.near_ptr[l]] != l)
      return fail(FMMBEM_ERR_INVALID, std::string(who) + "internal: a leaf whose row block is not its self block");
    const int tb = h.leaf_box[l];
    const int m = dof * (h.box_body_end[tb] - h.box_body_begin[tb]);
    max_m = std::max(max_m, m);
    off[(size_t)(l - h.leaf_begin) + 1] = off[(size_t)(l - h.leaf_begin)] + (int64_t)m * m;
  }
  if (max_m > kBlockInvMax)
    return fail(FMMBEM_ERR_UNSUPPORTED, std::string(who) + "a leaf holds " + std::to_string(max_m) + " unknowns; the kernels serve at most " +
                                            std::to_string(kBlockInvMax) + " (ncrit * dof)");
  DEVICE_SCOPE(plan->opts.device);
  fmmbem_plan::BlockInverse& bi = plan->binv;
  int* d_selfcol = nullptr;
  const int none = INT_MAX;
  int bad = none;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&bi.dev.val), sizeof(double) * (size_t)std::max<int64_t>(off.back(), 1));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(const_cast<int64_t**>(&bi.dev.off)), sizeof(int64_t) * off.size());
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&bi.dev.bad), sizeof(int));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_selfcol), sizeof(int) * std::max<size_t>(selfcol.size(), 1));
  if (e != hipSuccess) {
    if (d_selfcol) (void)hipFree(d_selfcol);
    plan->block_inverse_free();
    return fail(e == hipErrorOutOfMemory ? FMMBEM_ERR_ALLOC : FMMBEM_ERR_HIP, std::string(who) + hipGetErrorString(e));
  }
  hipStream_t s = plan->own_stream;
  e = hipMemcpy(const_cast<int64_t*>(bi.dev.off), off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(bi.dev.bad, &none, sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_selfcol, selfcol.data(), sizeof(int) * selfcol.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_blockinv_build(plan->d, bi.dev, d_selfcol, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemcpy(&bad, bi.dev.bad, sizeof(int), hipMemcpyDeviceToHost);
  (void)hipFree(d_selfcol);
  if (e != hipSuccess) { plan->block_inverse_free(); return fail(FMMBEM_ERR_HIP, std::string(who) + hipGetErrorString(e)); }
  if (bad != none) {                                   // the plan stays as it was: no inverse attached
    plan->block_inverse_free();
    const int tb = h.leaf_box[bad];
    return fail(FMMBEM_ERR_INVALID, std::string(who) + "leaf " + std::to_string(bad) + " (tree panels " + std::to_string(h.box_body_begin[tb]) + ".." +
                                        std::to_string(h.box_body_end[tb] - 1) + "): zero or non-finite pivot, its block is singular");
  }
  bi.max_m = max_m;
  bi.doubles = off.back();
  bi.built = true;
  return FMMBEM_OK;
}

int fmmbem_plan_block_inverse_apply_device(fmmbem_plan* plan, int k, const double* d_v, size_t ldv, double* d_z, size_t ldz, void* stream) {
  TRY(batch_args(plan, k, d_v, ldv, d_z, ldz));
  if (!plan->binv.built) return fail(FMMBEM_ERR_INVALID, "fmmbem_plan_block_inverse_apply: no inverse built on this plan (fmmbem_plan_block_inverse_build)");
  DEVICE_SCOPE(plan->opts.device);
  HIP_TRY(launch_blockinv_apply(plan->d, plan->binv.dev, plan->binv.max_m, k, d_v, ldv, d_z, ldz, static_cast<hipStream_t>(stream)));
  return FMMBEM_OK;
}

int fmmbem_plan_block_inverse_apply(fmmbem_plan* plan, int k, const double* v, size_t ldv, double* z, size_t ldz) {
  TRY(batch_args(plan, k, v, ldv, z, ldz));
  if (!plan->binv.built) return fail(FMMBEM_ERR_INVALID, "fmmbem_plan_block_inverse_apply: no inverse built on this plan (fmmbem_plan_block_inverse_build)");
  DEVICE_SCOPE(plan->opts.device);
  fmmbem_plan::BlockInverse& bi = plan->binv;
  const size_t n = (size_t)plan->hp.n * plan->d.dof;
  if (bi.stage_doubles < 2 * n * (size_t)k) {
    if (bi.stage) (void)hipFree(bi.stage);
    bi.stage = nullptr; bi.stage_doubles = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&bi.stage), sizeof(double) * 2 * n * (size_t)k));
    bi.stage_doubles = 2 * n * (size_t)k;
  }
  double *sv = bi.stage, *sz = bi.stage + n * (size_t)k;
  hipStream_t s = plan->own_stream;
  HIP_TRY(hipMemcpy2DAsync(sv, sizeof(double) * n, v, sizeof(double) * ldv, sizeof(double) * n, (size_t)k, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_blockinv_apply(plan->d, bi.dev, bi.max_m, k, sv, n, sz, n, s));
  HIP_TRY(hipMemcpy2DAsync(z, sizeof(double) * ldz, sz, sizeof(double) * n, sizeof(double) * n, (size_t)k, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FMMBEM_OK;
}

int fmmbem_plan_block_inverse_bytes(const fmmbem_plan* plan, int64_t* bytes) {
  if (!plan || !bytes) return fail(FMMBEM_ERR_INVALID, "null argument");
  *bytes = plan->binv.built ? plan->binv.doubles * (int64_t)sizeof(double) : 0;
  return FMMBEM_OK;
}

int fmmbem_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(FMMBEM_ERR_INVALID, "null buffer");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return FMMBEM_OK;
}

int fmmbem_host_unregister(void* ptr) {
  if (!ptr) return fail(FMMBEM_ERR_INVALID, "null buffer");
  HIP_TRY(hipHostUnregister(ptr));
  return FMMBEM_OK;
}

int fmmbem_plan_set_graphs(fmmbem_plan* plan, int enabled) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (plan->multi) { for (auto& sh : plan->multi->shards) sh->use_graphs = enabled != 0; return FMMBEM_OK; }
  plan->use_graphs = enabled != 0 && plan->on_device;
  return FMMBEM_OK;
}

int fmmbem_plan_set_timing(fmmbem_plan* plan, int enabled) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  if (plan->multi) { for (auto& sh : plan->multi->shards) TRY(fmmbem_plan_set_timing(sh.get(), enabled)); return FMMBEM_OK; }
  plan->timing = plan->on_device ? (enabled == 2 ? 2 : enabled != 0) : 0;
  plan->ev_count = 0;
  return FMMBEM_OK;
}

int fmmbem_plan_stats(const fmmbem_plan* plan, fmmbem_stats* o) {
  if (!plan || !o) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (plan->multi) {
    // the whole operator: what the shards own summed, the tree's figures from any of them, stage times the LONGEST shard's
    // (they run side by side), build times likewise
    const MultiDevice& m = *plan->multi;
    TRY(fmmbem_plan_stats(m.shards[0].get(), o));
    for (int r = 1; r < m.world(); ++r) {
      fmmbem_stats t;
      TRY(fmmbem_plan_stats(m.shards[r].get(), &t));
      o->near_nnz += t.near_nnz; o->m2l_pairs_owned += t.m2l_pairs_owned; o->near_bytes += t.near_bytes;
      o->near_side_entries += t.near_side_entries; o->near_recomputed_pairs += t.near_recomputed_pairs;
      o->m2m_ops = std::max(o->m2m_ops, t.m2m_ops); o->l2l_ops += t.l2l_ops; o->l2p_leaves += t.l2p_leaves; o->p2m_leaves += t.p2m_leaves;
      o->m2l_items += t.m2l_items; o->m2l_passes += t.m2l_passes;
      o->owned_leaf_end = t.owned_leaf_end; o->owned_row_end = t.owned_row_end;
      o->build_host_ms = std::max(o->build_host_ms, t.build_host_ms); o->build_assemble_ms = std::max(o->build_assemble_ms, t.build_assemble_ms);
      double* a[] = {&o->ms_total, &o->ms_gather, &o->ms_near, &o->ms_scatter, &o->ms_p2m, &o->ms_m2m, &o->ms_mh, &o->ms_m2l, &o->ms_l2l, &o->ms_l2p};
      const double b[] = {t.ms_total, t.ms_gather, t.ms_near, t.ms_scatter, t.ms_p2m, t.ms_m2m, t.ms_mh, t.ms_m2l, t.ms_l2l, t.ms_l2p};
      for (int k = 0; k < 10; ++k) *a[k] = std::max(*a[k], b[k]);
    }
    o->last_p = plan->last_p;
    o->n_devices = m.world();
    return FMMBEM_OK;
  }
  const HostPlan& h = plan->hp;
  std::memset(o, 0, sizeof(*o));
  o->n_panels = h.n; o->n_boxes = h.nboxes; o->n_leaves = h.nleaves(); o->n_levels = h.nlevels;
  o->near_nnz = h.near_nnz_owned; o->near_nnz_total = h.near_nnz_total;
  o->p2p_pairs = (int64_t)h.p2p_src.size(); o->m2l_pairs = (int64_t)h.lr_src.size(); o->m2l_pairs_owned = h.m2l_pairs_owned;
  o->m2m_ops = h.m2m_ops; o->l2l_ops = h.l2l_ops;
  o->l2l_reference_omitted = h.l2l_ref_omitted;
  o->p2m_leaves = (int64_t)h.p2m_leaves.size(); o->l2p_leaves = (int64_t)h.l2p_leaves.size();
  o->m2l_classes = (int64_t)h.m2l_class_rep.size() / 2;
  o->owned_leaf_begin = h.leaf_begin; o->owned_leaf_end = h.leaf_end;
  o->owned_row_begin = h.row_begin; o->owned_row_end = h.row_end;
  o->near_bytes = plan->g.near_bytes;
  const bool long_items = plan->last_p > 0 && m2l_rot_long_items(plan->last_p) && plan->g.use_rot(plan->last_p);   // the cut the last execute ran
  o->m2l_items = (int64_t)(long_items ? h.rot_item_ptr_long : h.rot_item_ptr).size() - 1;
  o->m2l_passes = long_items ? h.rot_passes_long : h.rot_passes;
  o->near_side_entries = plan->near_side_entries;
  o->near_recomputed_pairs = plan->g.near_recomputed_pairs;
  o->near_f32_bytes = plan->d.near_f32 ? plan->g.near_f32_floats * (int64_t)sizeof(float) : 0;
  o->last_near_f32 = plan->last_near_f32;
  o->geometry_shared = (int32_t)plan->shared.use_count();
  o->n_devices = 1;
  o->expansion_slots = plan->on_device ? plan->d.nslots : (plan->opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 8 : 2);
  o->m2l_kernel = plan->last_p > 0 ? (plan->treecode() ? 4 : plan->g.use_rot(plan->last_p) ? 1 : plan->last_p <= 4 ? 3 : 2) : 0;
  o->rot_nop_orders = (int64_t)rot_nop_orders_m2l() | ((int64_t)rot_nop_orders_m2m() << 16) | ((int64_t)rot_nop_orders_l2l() << 32);
  o->tree_coder_levels = h.tree_levels_max;
  o->expansions_active = (plan->has_bc[0] ? 1 : 0) | (plan->has_bc[1] ? 2 : 0);
  o->last_p = plan->last_p;
  o->build_host_ms = plan->build_host_ms; o->build_assemble_ms = plan->build_assemble_ms;
  if (plan->targets) {                                 // the source tree's figures (the target tree's: fmmbem_plan_target_info)
    o->n_panels = h.n_src;
    o->n_boxes = (int64_t)h.src_box.size(); o->n_leaves = h.src_nleaves; o->n_levels = h.src_nlevels;
    o->owned_leaf_begin = 0; o->owned_leaf_end = h.tgt_nleaves;
    o->owned_row_begin = 0; o->owned_row_end = h.n - h.n_src;
  }
  if (plan->on_device && plan->ev_count > 0) {
    // mean stage times over the recorded executes (waits for the recorded events)
    using Stage = fmmbem_plan::Stage;
    constexpr int NS = fmmbem_plan::kStages, NR = fmmbem_plan::kRing;
    const int64_t have = plan->ev_count < NR ? plan->ev_count : NR;
    double sum[NS + 1] = {0};
    int64_t used = 0;
    DEVICE_SCOPE(plan->opts.device);
    for (int64_t i = 0; i < have; ++i) {
      const int64_t slot = (plan->ev_count - 1 - i) % NR;
      const hipEvent_t* set = &plan->ev[(size_t)slot * 2 * NS];
      const unsigned mask = plan->ev_mask[slot];
      int last = -1, first = -1;
      for (int k = 0; k < NS; ++k) if (mask & (1u << k)) { last = k; if (first < 0) first = k; }
      if (mask & (1u << (int)Stage::Scatter)) last = (int)Stage::Scatter;     // the delivery of the result is the last thing an execute does
      if (last < 0) continue;
      float f = 0;
      for (int k = 0; k < NS; ++k) {
        if (!(mask & (1u << k))) continue;
        HIP_TRY(hipEventSynchronize(set[2 * k + 1]));
        HIP_TRY(hipEventElapsedTime(&f, set[2 * k], set[2 * k + 1]));
        sum[k] += f;
      }
      HIP_TRY(hipEventElapsedTime(&f, set[2 * first], set[2 * last + 1]));      // both on the caller's stream
      sum[NS] += f;
      ++used;
    }
    if (used) {
      const double inv = 1.0 / double(used);
      auto mean = [&](Stage k) { return sum[(int)k] * inv; };
      o->ms_gather = mean(Stage::Gather); o->ms_near = mean(Stage::Spmv); o->ms_scatter = mean(Stage::Scatter); o->ms_p2m = mean(Stage::P2M);
      o->ms_m2m = mean(Stage::M2M); o->ms_mh = mean(Stage::Mh); o->ms_m2l = mean(Stage::M2L); o->ms_l2l = mean(Stage::L2L);
      o->ms_l2p = mean(Stage::L2P); o->ms_total = sum[NS] * inv;
      o->timed_executes = used;
    }
  }
  return FMMBEM_OK;
}

int fmmbem_plan_get_perm(const fmmbem_plan* plan, uint32_t* out) {
  if (!plan || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  std::memcpy(out, plan->hp.perm.data(), sizeof(uint32_t) * (size_t)(plan->targets ? plan->hp.n_src : plan->hp.n));
  return FMMBEM_OK;
}

int fmmbem_plan_get_boxes(const fmmbem_plan* plan, double* center, double* side, int32_t* level, int32_t* is_leaf,
                          int32_t* parent, int32_t* body_begin, int32_t* body_end) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  const HostPlan& h = plan->hp;
  if (plan->targets) { dual_boxes(h, false, center, side, level, is_leaf, parent, body_begin, body_end); return FMMBEM_OK; }
  for (int b = 0; b < h.nboxes; ++b) {
    if (center) std::memcpy(center + 3 * b, &h.box_center[3 * b], sizeof(double) * 3);
    if (side) side[b] = h.box_side[b];
    if (level) level[b] = h.box_level[b];
    if (is_leaf) is_leaf[b] = h.box_leaf[b];
    if (parent) parent[b] = h.box_parent[b];
    if (body_begin) body_begin[b] = h.box_body_begin[b];
    if (body_end) body_end[b] = h.box_body_end[b];
  }
  return FMMBEM_OK;
}

int fmmbem_plan_get_pairs(const fmmbem_plan* plan, int which, int32_t* out, int64_t* n) {
  if (!plan || !n) return fail(FMMBEM_ERR_INVALID, "null argument");
  const HostPlan& h = plan->hp;
  std::vector<int32_t> flat;
  // a target plan: the boxes of a pair in their own tree's numbering (source box, target box), as fmmbem_plan_get_boxes /
  // fmmbem_plan_get_target_boxes number them
  std::vector<int> loc;
  if (plan->targets) {
    loc.assign((size_t)h.nboxes, -1);
    for (size_t b = 0; b < h.src_box.size(); ++b) loc[(size_t)h.src_box[b]] = (int)b;
    for (size_t b = 0; b < h.tgt_box.size(); ++b) loc[(size_t)h.tgt_box[b]] = (int)b;
  }
  auto L = [&](int b) { return loc.empty() ? b : loc[(size_t)b]; };
  switch (which) {
    case 0: for (size_t i = 0; i < h.p2p_src.size(); ++i) { flat.push_back(L(h.p2p_src[i])); flat.push_back(L(h.p2p_tgt[i])); } break;
    case 1: for (size_t i = 0; i < h.lr_src.size(); ++i) { flat.push_back(L(h.lr_src[i])); flat.push_back(L(h.lr_tgt[i])); } break;
    case 2:
      for (int par : h.m2m_parents)
        for (int c = h.box_child_begin[par]; c < h.box_child_end[par]; ++c) { flat.push_back(L(c)); flat.push_back(L(par)); }
      break;
    case 3: for (int c : h.l2l_children) { flat.push_back(L(h.box_parent[c])); flat.push_back(L(c)); } break;
    case 4:
      if (h.rot_alias) {
        for (int b = 0; b < h.nboxes; ++b)
          for (int i = h.m2l_ptr[b]; i < h.m2l_ptr[b + 1]; ++i) { flat.push_back(L(h.m2l_src[i])); flat.push_back(L(b)); }
      } else
        for (size_t i = 0; i < h.rot_src.size(); ++i) { flat.push_back(L(h.rot_src[i])); flat.push_back(L(h.rot_tgt[i])); }
      break;
    case 5: for (size_t i = 0; i + 1 < h.rot_item_ptr.size(); ++i) { flat.push_back(h.rot_item_ptr[i]); flat.push_back(h.rot_item_ptr[i + 1]); } break;
    case 6: for (size_t i = 0; i + 1 < h.rot_item_ptr_long.size(); ++i) { flat.push_back(h.rot_item_ptr_long[i]); flat.push_back(h.rot_item_ptr_long[i + 1]); } break;
    default: return fail(FMMBEM_ERR_INVALID, "which must be 0..6");
  }
  *n = (int64_t)flat.size() / 2;
  if (out) std::memcpy(out, flat.data(), flat.size() * sizeof(int32_t));
  return FMMBEM_OK;
}

int fmmbem_plan_get_near_row(const fmmbem_plan* plan, int64_t row, uint32_t* cols, double* vals, int64_t* n) {
  TRY(target_plan_only(plan, "fmmbem_plan_get_near_row"));
  if (!plan || !n) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (plan->multi) {
    const MultiDevice& m = *plan->multi;
    const int64_t prow = row / plan->d.dof;
    for (int r = 0; r < m.world(); ++r)
      if (prow >= m.cut[r] && prow < m.cut[r + 1]) return fmmbem_plan_get_near_row(m.shards[r].get(), row, cols, vals, n);
    return fail(FMMBEM_ERR_INVALID, "row out of range");
  }
  const HostPlan& h = plan->hp;
  const int dof = plan->opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1;
  const int64_t prow = row / dof;                      // panel row (tree order); row counts unknowns
  const int comp = (int)(row % dof);
  if (prow < h.row_begin || prow >= h.row_end) return fail(FMMBEM_ERR_INVALID, "row not owned by this shard");
  // owning leaf: last leaf whose first row <= prow
  int lo = h.leaf_begin, hi = h.leaf_end - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (h.box_body_begin[h.leaf_box[mid]] <= prow) lo = mid; else hi = mid - 1;
  }
  const int leaf = lo, tb = h.leaf_box[leaf];
  const int ncols = dof * h.near_ncols[leaf];
  *n = ncols;
  if (cols) {
    int at = 0;
    for (int64_t s = h.near_ptr[leaf]; s < h.near_ptr[leaf + 1]; ++s) {
      const int sb = h.leaf_box[h.near_src[s]];
      for (int j = h.box_body_begin[sb]; j < h.box_body_end[sb]; ++j)
        for (int b = 0; b < dof; ++b) cols[at++] = (uint32_t)(dof * j + b);
    }
  }
  if (vals) {
    if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "near values live on the device");
    if (!plan->opts.sparse_local) return fail(FMMBEM_ERR_INVALID, "matrix-free plan holds no near matrix");
    DEVICE_SCOPE(plan->opts.device);
    if (!plan->g.near_rec_host.empty() && plan->g.near_rec_host[leaf]) {
      // hybrid plan, recomputed leaf: no block is stored -- the row is evaluated now, by the entry functions of the assembly
      const int ncp = h.near_ncols[leaf];
      std::vector<int> pcol((size_t)ncp);
      int at = 0;
      for (int64_t s = h.near_ptr[leaf]; s < h.near_ptr[leaf + 1]; ++s) {
        const int sb = h.leaf_box[h.near_src[s]];
        for (int j = h.box_body_begin[sb]; j < h.box_body_end[sb]; ++j) pcol[at++] = j;
      }
      int* d_col = nullptr;
      double* d_val = nullptr;
      HIP_TRY(hipMalloc(&d_col, sizeof(int) * (size_t)ncp));
      if (hipMalloc(&d_val, sizeof(double) * (size_t)ncp * dof * dof) != hipSuccess) { (void)hipFree(d_col); return fail(FMMBEM_ERR_ALLOC, "device allocation failed"); }
      std::vector<double> blk((size_t)ncp * dof * dof);
      hipError_t e = hipMemcpy(d_col, pcol.data(), sizeof(int) * (size_t)ncp, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = launch_near_row_eval(plan->d, prow, d_col, ncp, d_val, plan->own_stream);
      if (e == hipSuccess) e = hipStreamSynchronize(plan->own_stream);
      if (e == hipSuccess) e = hipMemcpy(blk.data(), d_val, sizeof(double) * blk.size(), hipMemcpyDeviceToHost);
      (void)hipFree(d_col); (void)hipFree(d_val);
      if (e != hipSuccess) return fail(FMMBEM_ERR_HIP, hipGetErrorString(e));
      for (int c = 0; c < ncp; ++c)
        for (int b = 0; b < dof; ++b) vals[dof * c + b] = blk[(size_t)c * dof * dof + comp * dof + b];
      return FMMBEM_OK;
    }
    const int64_t off = plan->g.near_off_host[leaf];
    if (plan->d.near_sym) {                            // Stokes, symmetric blocks: expand row `comp` of the panel row's 3x3 blocks
      const int ncp = h.near_ncols[leaf];
      const int64_t soff = plan->g.sym_off_host[leaf];
      std::vector<double> six((size_t)6 * ncp);
      HIP_TRY(hipMemcpy(six.data(), plan->d.near_sym + soff + (prow - h.box_body_begin[tb]) * 6 * ncp, sizeof(double) * six.size(), hipMemcpyDeviceToHost));
      const double *p0 = six.data(), *p1 = p0 + 2 * ncp, *p2 = p1 + 2 * ncp;      // (xx,xy) (xz,yy) (yz,zz) per source panel
      for (int c = 0; c < ncp; ++c) {
        const double m[3][3] = {{p0[2 * c], p0[2 * c + 1], p1[2 * c]}, {p0[2 * c + 1], p1[2 * c + 1], p2[2 * c]}, {p1[2 * c], p2[2 * c], p2[2 * c + 1]}};
        for (int b = 0; b < 3; ++b) vals[3 * c + b] = m[comp][b];
      }
      return FMMBEM_OK;
    }
    const int stride = (ncols + 1) & ~1;
    const int64_t r = (prow - h.box_body_begin[tb]) * dof + comp;
    HIP_TRY(hipMemcpy(vals, plan->d.near_val + off + r * stride, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  }
  return FMMBEM_OK;
}

int fmmbem_plan_get_diagonal(const fmmbem_plan* plan, double* out) {
  TRY(target_plan_only(plan, "fmmbem_plan_get_diagonal"));
  if (!plan || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (plan->multi) {                                   // every shard returns its own rows and zeros elsewhere
    const MultiDevice& m = *plan->multi;
    const size_t nd = (size_t)plan->hp.n * plan->d.dof;
    std::vector<double> part(nd);
    std::fill(out, out + nd, 0.0);
    for (int r = 0; r < m.world(); ++r) {
      TRY(fmmbem_plan_get_diagonal(m.shards[r].get(), part.data()));
      for (size_t i = 0; i < nd; ++i) out[i] += part[i];
    }
    return FMMBEM_OK;
  }
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "near values live on the device");
  if (!plan->opts.sparse_local) return fail(FMMBEM_ERR_INVALID, "matrix-free plan holds no near matrix");
  const HostPlan& h = plan->hp;
  const int dof = plan->d.dof;
  DEVICE_SCOPE(plan->opts.device);
  std::vector<int> selfcol(h.nleaves(), 0);
  for (int l = h.leaf_begin; l < h.leaf_end; ++l) {
    int col = 0;
    bool found = false;
    for (int64_t s = h.near_ptr[l]; s < h.near_ptr[l + 1]; ++s) {
      if (h.near_src[s] == l) { found = true; break; }
      const int sb = h.leaf_box[h.near_src[s]];
      col += h.box_body_end[sb] - h.box_body_begin[sb];
    }
    if (!found) return fail(FMMBEM_ERR_INVALID, "internal: a leaf without its self block");
    selfcol[l] = dof * col;
  }
  int* d_sc = nullptr;
  double* d_out = nullptr;
  const size_t nb = sizeof(double) * (size_t)h.n * dof;
  HIP_TRY(hipMalloc(&d_sc, sizeof(int) * selfcol.size()));
  if (hipMalloc(&d_out, nb) != hipSuccess) { (void)hipFree(d_sc); return fail(FMMBEM_ERR_ALLOC, "device allocation failed"); }
  hipError_t e = hipMemcpy(d_sc, selfcol.data(), sizeof(int) * selfcol.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, nb);                       // rows of other shards stay zero
  if (e == hipSuccess) e = launch_near_diag(plan->d, d_sc, d_out, plan->own_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(plan->own_stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, nb, hipMemcpyDeviceToHost);
  (void)hipFree(d_sc); (void)hipFree(d_out);
  if (e != hipSuccess) return fail(FMMBEM_ERR_HIP, hipGetErrorString(e));
  return FMMBEM_OK;
}

int fmmbem_plan_get_expansions(const fmmbem_plan* plan, int which, int p, double* out) {
  TRY(shard_entry(plan, "fmmbem_plan_get_expansions", "null argument"));
  if (!out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (which != 0 && plan->treecode()) return fail(FMMBEM_ERR_UNSUPPORTED, "a treecode plan holds no local expansions (M only)");
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "expansions live on the device");
  if (p < 1 || p > plan->hp.opt.p_max) return fail(FMMBEM_ERR_INVALID, "p outside [1, p_max]");
  DEVICE_SCOPE(plan->opts.device);
  const DevicePlan& d = plan->d;
  const int ns = d.nslots;
  std::vector<double2> tmp((size_t)d.nboxes * ns * d.s_max);
  HIP_TRY(hipMemcpy(tmp.data(), which == 0 ? d.M : d.L, tmp.size() * sizeof(double2), hipMemcpyDeviceToHost));
  const int S = p * (p + 1) / 2;
  for (int b = 0; b < d.nboxes; ++b)
    for (int s = 0; s < ns; ++s)
      for (int i = 0; i < S; ++i) {
        const double2 v = tmp[((size_t)b * ns + s) * d.s_max + i];
        out[(((size_t)b * ns + s) * S + i) * 2] = v.x;
        out[(((size_t)b * ns + s) * S + i) * 2 + 1] = v.y;
      }
  return FMMBEM_OK;
}

int fmmbem_kernel_entries(const fmmbem_options* opts, size_t n, const double* target_vertices, const uint8_t* target_bc,
                          const double* source_vertices, double* out) {
  if (!opts || !target_vertices || !source_vertices || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (opts->kernel != FMMBEM_KERNEL_LAPLACE_BEM && opts->kernel != FMMBEM_KERNEL_STOKES_BEM)
    return fail(FMMBEM_ERR_UNSUPPORTED, "unknown kernel id");
  if (n == 0) return FMMBEM_OK;
  if (n > ((size_t)1 << 30)) return fail(FMMBEM_ERR_INVALID, "too many pairs");
  const bool stokes = opts->kernel == FMMBEM_KERNEL_STOKES_BEM;
  QuadRule rule, fine;
  if (!quad_rule(opts->quad_k, rule)) return fail(FMMBEM_ERR_INVALID, "invalid quadrature key (valid: 1 3 4 7 13 17 19 25 79)");
  if (stokes) {
    if (!quad_rule(opts->quad_k_fine, fine)) return fail(FMMBEM_ERR_INVALID, "invalid K_fine (valid: 1 3 4 7 13 17 19 25 79)");
    if (!(opts->mu > 0)) return fail(FMMBEM_ERR_INVALID, "Stokes: viscosity mu must be positive");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMMBEM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU execution path)");
  if (opts->device < 0 || opts->device >= ndev) return fail(FMMBEM_ERR_INVALID, "device ordinal out of range");
  DEVICE_SCOPE(opts->device);
  const int64_t N = 2 * (int64_t)n;
  PanelSoA P;
  try {
    alloc_panels(P, N, rule.n);
  } catch (const std::bad_alloc&) {
    return fail(FMMBEM_ERR_ALLOC, "host allocation failed");
  }
  for (size_t i = 0; i < n; ++i) {
    fill_panel(P, N, (int64_t)i, target_vertices + 9 * i, rule, target_bc ? (target_bc[i] ? 1 : 0) : 0);
    fill_panel(P, N, (int64_t)(n + i), source_vertices + 9 * i, rule, 0);
  }
  struct Frees {
    std::vector<void*> v;
    ~Frees() { for (void* p : v) (void)hipFree(p); }
  } frees;
  auto up = [&](const void* src, size_t bytes, const void** dst) -> hipError_t {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) return e;
    frees.v.push_back(p);
    *dst = p;
    return bytes ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  DevicePlan d{};
  d.n = N; d.nq = rule.n; d.kernel = opts->kernel; d.dof = stokes ? 3 : 1; d.mu = opts->mu;
  for (int q = 0; q < rule.n; ++q) d.qw[q] = rule.w[q];
  std::vector<double> qf((size_t)fine.n * 4);
  if (stokes) {
    d.nqf = fine.n;
    for (int q = 0; q < fine.n; ++q) { for (int k = 0; k < 3; ++k) qf[4 * q + k] = fine.pts[q][k]; qf[4 * q + 3] = fine.w[q]; }
  }
#define UP(field, vec) HIP_TRY(up(vec.data(), vec.size() * sizeof(vec[0]), reinterpret_cast<const void**>(&d.field)))
  UP(cx, P.cx); UP(cy, P.cy); UP(cz, P.cz); UP(nx, P.nx); UP(ny, P.ny); UP(nz, P.nz);
  UP(area, P.area); UP(quad, P.quad); UP(vert, P.vert); UP(bc, P.bc);
  if (stokes) UP(qf, qf);
#undef UP
  const size_t per = stokes ? 9 : 1;
  double* d_out = nullptr;
  HIP_TRY(hipMalloc(&d_out, sizeof(double) * n * per));
  frees.v.push_back(d_out);
  HIP_TRY(launch_kernel_entries(d, (int)n, d_out, nullptr));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * n * per, hipMemcpyDeviceToHost));
  return FMMBEM_OK;
}

// The pair functions of the field quantities for n independent pairs, in the layout of fmmbem_kernel_entries: panels [0, n) the
// targets, [n, 2n) the sources.  Laplace: the normals and the flags go up; Stokes: the fine rule.
static int field_entries(FieldQuantity q, const fmmbem_options* opts, size_t n, const double* target_vertices, const uint8_t* target_bc,
                         const double* source_vertices, double* out) {
  const FieldRow& row = kField[(int)q];
  if (!opts || !target_vertices || !source_vertices || !out) return fail(FMMBEM_ERR_INVALID, "null argument");
  if (opts->kernel != (row.stokes ? FMMBEM_KERNEL_STOKES_BEM : FMMBEM_KERNEL_LAPLACE_BEM)) return fail(FMMBEM_ERR_UNSUPPORTED, row.entries_kernel);
  if (n == 0) return FMMBEM_OK;
  if (n > row.max_pairs) return fail(FMMBEM_ERR_INVALID, "too many pairs");
  QuadRule rule, fine;
  if (!quad_rule(opts->quad_k, rule)) return fail(FMMBEM_ERR_INVALID, "invalid quadrature key (valid: 1 3 4 7 13 17 19 25 79)");
  if (row.stokes && !quad_rule(opts->quad_k_fine, fine)) return fail(FMMBEM_ERR_INVALID, "invalid K_fine (valid: 1 3 4 7 13 17 19 25 79)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMMBEM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU execution path)");
  if (opts->device < 0 || opts->device >= ndev) return fail(FMMBEM_ERR_INVALID, "device ordinal out of range");
  DEVICE_SCOPE(opts->device);
  const int64_t N = 2 * (int64_t)n;
  PanelSoA P;
  std::vector<double> qf((size_t)fine.n * 4);
  try {
    alloc_panels(P, N, rule.n);
  } catch (const std::bad_alloc&) {
    return fail(FMMBEM_ERR_ALLOC, "host allocation failed");
  }
  for (size_t i = 0; i < n; ++i) {
    fill_panel(P, N, (int64_t)i, target_vertices + 9 * i, rule, target_bc ? (target_bc[i] ? 1 : 0) : 0);
    fill_panel(P, N, (int64_t)(n + i), source_vertices + 9 * i, rule, 0);
  }
  for (int k = 0; k < fine.n; ++k) { for (int c = 0; c < 3; ++c) qf[4 * k + c] = fine.pts[k][c]; qf[4 * k + 3] = fine.w[k]; }
  Scratch mem;
  DevicePlan d{};
  d.n = N; d.nq = rule.n; d.kernel = opts->kernel; d.dof = row.stokes ? 3 : 1;
  for (int k = 0; k < rule.n; ++k) d.qw[k] = rule.w[k];
  TRY(mem.up(P.cx.data(), P.cx.size(), &d.cx)); TRY(mem.up(P.cy.data(), P.cy.size(), &d.cy)); TRY(mem.up(P.cz.data(), P.cz.size(), &d.cz));
  TRY(mem.up(P.area.data(), P.area.size(), &d.area)); TRY(mem.up(P.quad.data(), P.quad.size(), &d.quad));
  TRY(mem.up(P.vert.data(), P.vert.size(), &d.vert));
  if (row.stokes) {
    d.nqf = fine.n; d.mu = opts->mu;
    TRY(mem.up(qf.data(), qf.size(), &d.qf));
  } else {
    TRY(mem.up(P.nx.data(), P.nx.size(), &d.nx)); TRY(mem.up(P.ny.data(), P.ny.size(), &d.ny)); TRY(mem.up(P.nz.data(), P.nz.size(), &d.nz));
    TRY(mem.up(P.bc.data(), P.bc.size(), &d.bc));
  }
  double* d_out = nullptr;
  TRY(mem.alloc(row.entry_width * n, &d_out));
  HIP_TRY(launch_field_entries(q, d, (int)n, d_out, nullptr));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * row.entry_width * n, hipMemcpyDeviceToHost));
  return FMMBEM_OK;
}

int fmmbem_kernel_gradient_entries(const fmmbem_options* opts, size_t n, const double* target_vertices, const uint8_t* target_bc,
                                   const double* source_vertices, double* out) {
  return field_entries(FieldQuantity::Gradient, opts, n, target_vertices, target_bc, source_vertices, out);
}
int fmmbem_kernel_hessian_entries(const fmmbem_options* opts, size_t n, const double* target_vertices, const uint8_t* target_bc,
                                  const double* source_vertices, double* out) {
  return field_entries(FieldQuantity::Hessian, opts, n, target_vertices, target_bc, source_vertices, out);
}
int fmmbem_kernel_pressure_entries(const fmmbem_options* opts, size_t n, const double* target_vertices, const double* source_vertices,
                                   double* out) {
  return field_entries(FieldQuantity::Pressure, opts, n, target_vertices, nullptr, source_vertices, out);
}
int fmmbem_kernel_velocity_gradient_entries(const fmmbem_options* opts, size_t n, const double* target_vertices,
                                            const double* source_vertices, double* out) {
  return field_entries(FieldQuantity::VelocityGradient, opts, n, target_vertices, nullptr, source_vertices, out);
}

int fmmbem_mesh_unit_sphere(int recursions, double* vertices, size_t* n_panels) {
  if (recursions < 1 || recursions > 12 || !n_panels) return fail(FMMBEM_ERR_INVALID, "recursions must be 1..12");
  *n_panels = (size_t)unit_sphere(recursions, vertices);
  return FMMBEM_OK;
}

const char* fmmbem_status_string(int status) {
  switch (status) {
    case FMMBEM_OK: return "ok";
    case FMMBEM_ERR_INVALID: return "invalid argument";
    case FMMBEM_ERR_NO_DEVICE: return "no HIP device";
    case FMMBEM_ERR_HIP: return "HIP runtime error";
    case FMMBEM_ERR_ALLOC: return "allocation failed";
    case FMMBEM_ERR_TREE: return "octree too deep";
    case FMMBEM_ERR_UNSUPPORTED: return "unsupported option";
    case FMMBEM_ERR_IO: return "file input/output error";
    default: return "unknown status";
  }
}

const char* fmmbem_last_error(void) { return g_last_error.c_str(); }
int fmmbem_version(void) { return FMMBEM_VERSION; }

}  // extern "C"

// ---- the first layout of fmmbem_options (include/fmmbem.h: 120 bytes, no stokes_batch_width) under the plain names ----
// Programs compiled against the earlier header call these: the struct they hold ends where stokes_batch_width begins, so nothing
// here reads or writes past it; the field is taken as 0.
#undef fmmbem_options_default
#undef fmmbem_plan_create
#undef fmmbem_plan_create_targets
#undef fmmbem_kernel_entries
#undef fmmbem_ops_create
#undef fmmbem_direct_create
static constexpr size_t kOptionsR1 = offsetof(fmmbem_options, stokes_batch_width);
static_assert(kOptionsR1 == 120 && sizeof(fmmbem_options) == 128, "layouts of fmmbem_options (include/fmmbem.h)");
struct OptionsR1 {                                     // the caller's 120 bytes widened to today's struct
  fmmbem_options o;
  const fmmbem_options* p;
  explicit OptionsR1(const fmmbem_options* r1) : p(r1 ? &o : nullptr) {
    std::memset(&o, 0, sizeof(o));
    if (r1) std::memcpy(&o, r1, kOptionsR1);
  }
};
extern "C" {
void fmmbem_options_default(fmmbem_options* o) {
  if (!o) return;
  fmmbem_options full;
  fmmbem_options_default_r2(&full);
  std::memcpy(o, &full, kOptionsR1);
}
int fmmbem_plan_create(const fmmbem_options* opts, size_t n_panels, const double* vertices, const uint8_t* bc, fmmbem_plan** out) {
  return fmmbem_plan_create_r2(OptionsR1(opts).p, n_panels, vertices, bc, out);
}
int fmmbem_plan_create_targets(const fmmbem_options* opts, size_t n_panels, const double* vertices, const uint8_t* bc,
                               size_t n_targets, const double* target_points, const uint8_t* target_bc, fmmbem_plan** out) {
  return fmmbem_plan_create_targets_r2(OptionsR1(opts).p, n_panels, vertices, bc, n_targets, target_points, target_bc, out);
}
int fmmbem_kernel_entries(const fmmbem_options* opts, size_t n, const double* target_vertices, const uint8_t* target_bc,
                          const double* source_vertices, double* out) {
  return fmmbem_kernel_entries_r2(OptionsR1(opts).p, n, target_vertices, target_bc, source_vertices, out);
}
int fmmbem_ops_create(const fmmbem_options* opts, fmmbem_ops** out) { return fmmbem_ops_create_r2(OptionsR1(opts).p, out); }
int fmmbem_direct_create(const fmmbem_options* opts, size_t n_sources, const double* source_vertices, fmmbem_direct** out) {
  return fmmbem_direct_create_r2(OptionsR1(opts).p, n_sources, source_vertices, out);
}
}  // extern "C"

// what the solver of krylov.hip needs to know about a plan; it reaches the matvec through the public entry point
int fmmbem::plan_solver_info(fmmbem_plan* plan, int* device, int64_t* unknowns, int* p_max, fmmbem::SolverWs*** slot) {
  if (!plan) return fail(FMMBEM_ERR_INVALID, "null plan");
  TRY(target_plan_only(plan, "fmmbem_gmres"));
  if (!plan->on_device) return fail(FMMBEM_ERR_NO_DEVICE, "plan was built host-only; there is no CPU execution path");
  if (!plan->multi && (plan->result_slices || plan->hp.opt.shard_world > 1))
    return fail(FMMBEM_ERR_UNSUPPORTED, "fmmbem_gmres runs on a whole operator; shards are driven by the caller's collectives (distributed.py)");
  *device = plan->opts.device;
  *unknowns = (int64_t)plan->hp.n * (plan->opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1);
  *p_max = plan->hp.opt.p_max;
  *slot = &plan->solver_ws;
  return FMMBEM_OK;
}

// doubles of one x vector of the plan: what the batched solver checks its leading dimensions against before anything else
// kind 3 of fmmbem_preconditioner: has fmmbem_plan_block_inverse_build succeeded on this plan?
bool fmmbem::plan_block_inverse_built(const fmmbem_plan* plan) { return plan && plan->binv.built; }

size_t fmmbem::plan_unknowns(const fmmbem_plan* plan) {
  return (size_t)(plan->targets ? plan->hp.n_src : plan->hp.n) * (plan->opts.kernel == FMMBEM_KERNEL_STOKES_BEM ? 3 : 1);
}
