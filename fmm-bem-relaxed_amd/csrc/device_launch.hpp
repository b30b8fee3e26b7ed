// device_launch.hpp -- prototypes of the kernel launchers (kernels_near.hip, kernels_far.hip, kernels_m2l.hip and the three
// builds of kernels_m2l_rot.hip).  Kept apart from device_plan.hpp (the structs the kernels take by value) so that adding a
// launcher does not rebuild the rotation kernels, four minutes each.
#pragma once
#include "device_plan.hpp"
#include "shift_lanes.hpp"

namespace fmmbem {

// ---- launchers (kernels_near.hip / kernels_far.hip); all asynchronous on `s` ----
hipError_t launch_near_assemble(const DevicePlan& d, hipStream_t s);
hipError_t launch_gather_x(const DevicePlan& d, const double* x, hipStream_t s);
hipError_t launch_near_spmv(const DevicePlan& d, hipStream_t s);
// float near field (fmmbem_options.near_f32_max_p; the plans it serves: near_f32_ok, launch_choice.hpp): the copy of the stored
// values into DevicePlan::near_f32 (after the assembly); the pass that streams it instead of launch_near_spmv
hipError_t launch_near_to_f32(const DevicePlan& d, hipStream_t s);
hipError_t launch_near_spmv_f32(const DevicePlan& d, hipStream_t s);
struct HybridStreams { hipStream_t recompute = nullptr; hipEvent_t fork = nullptr, join_recompute = nullptr; };
hipError_t launch_near_hybrid(const DevicePlan& d, hipStream_t s, const HybridStreams& hs);   // near_stream_fraction < 1
hipError_t launch_kernel_entries(const DevicePlan& d, int m, double* out, hipStream_t s);   // panels [0,m) targets, [m,2m) sources
hipError_t launch_panel_setup(int64_t n, const uint32_t* perm, const double* v_orig, int nq, const double* pts, double* cx, double* cy,
                              double* cz, double* nx, double* ny, double* nz, double* area, double* quad, double* vert, hipStream_t s);
int rcg_item_rows();
hipError_t launch_rc_pack(const DevicePlan& d, double* rc_src, double* rc_nrm, hipStream_t s);
hipError_t launch_near_row_eval(const DevicePlan& d, int64_t prow, const int* cols, int n, double* out, hipStream_t s);
hipError_t launch_near_diag(const DevicePlan& d, const int* selfcol, double* out, hipStream_t s);
hipError_t launch_near_matfree(const DevicePlan& d, hipStream_t s);
hipError_t launch_mf_side(const DevicePlan& d, int phase, int* side_cnt, const int64_t* side_ptr, int* side_col, const int* side_row,
                          double* side_val, int64_t nside, hipStream_t s);
hipError_t launch_scatter_y(const DevicePlan& d, double* y, hipStream_t s);
hipError_t launch_assemble_slices(const DevicePlan& d, const double* slices, double* y, int world, const int64_t* d_cut, int64_t chunk,
                                  hipStream_t s);
hipError_t launch_p2m(const DevicePlan& d, int p, hipStream_t s);
// kernels_near.hip: launch_near_spmv and launch_p2m as ONE grid, the P2M workgroups queued behind the near field's -- bit for bit
// the two launches; only the plans and orders at which those take near_spmv_pipe_kernel and p2m_stream_kernel (near_p2m_ok,
// launch_choice.hpp)
hipError_t launch_near_p2m(const DevicePlan& d, int p, hipStream_t s);
hipError_t launch_p2m_table(const DevicePlan& d, double2* tab, hipStream_t s);
hipError_t launch_p2m_table_grad(const DevicePlan& d, double2* tab, hipStream_t s);     // one-off: fills DevicePlan::p2m_tab's storage
hipError_t launch_m2m_level(const DevicePlan& d, const ShiftOpDev& op, int p, int first, int count, hipStream_t s);
// multipoles of the boxes a shard owns -> send buffer [idx][active slot][S(p)]; all shards' buffers -> M (own slice skipped)
hipError_t launch_xch_pack(const DevicePlan& d, int p, double2* send, hipStream_t s);
hipError_t launch_xch_unpack(const DevicePlan& d, int p, const double2* recv, hipStream_t s);
hipError_t launch_mh_prep(const DevicePlan& d, int p, hipStream_t s);
// d_dev: a copy of d in device memory (the M2L kernel re-reads the plan fields it needs with scalar loads every source
// instead of keeping them alive in SGPRs across its FMA region)
hipError_t launch_m2l(const DevicePlan& d, const DevicePlan* d_dev, int p, hipStream_t s);
bool m2l_rot_supported(int p);
bool shift_rot_supported(int p);
hipError_t launch_m2m_rot(const DevicePlan& d, const RotWork& w, int p, hipStream_t s);   // M[tgt = parent] = sum over its children
hipError_t launch_l2l_rot(const DevicePlan& d, const RotWork& w, int p, hipStream_t s);   // L[tgt = child] += shift of L[src = parent]
hipError_t launch_m2l_rot(const DevicePlan& d, const DevicePlan* d_dev, int p, hipStream_t s);
bool m2l_rot_long_items(int p);
// kernels_shift.hip: the tree passes with one pair per wavefront (lane = coefficient); bit for bit the one-pair-per-lane kernels' results
bool shift_lanes_supported(int p);
hipError_t launch_m2m_lanes(const DevicePlan& d, const ShiftLaneWork& w, int p, hipStream_t s);
hipError_t launch_l2l_lanes(const DevicePlan& d, const ShiftLaneWork& w, int p, hipStream_t s);
// bit p - 1: orders of the four rotation objects that carry "s_nop 1" in front of their DPP FMAs (csrc/Makefile ROTBUILD)
unsigned rot_nop_orders_m2l();
unsigned rot_nop_orders_m2m();
unsigned rot_nop_orders_l2l();
int l2p_group_leaves(int kernel);                      // most leaves an L2P work group may hold (the kernels' LDS slice per wavefront)
hipError_t launch_m2l_rot_zero(const DevicePlan& d, int p, hipStream_t s);
hipError_t launch_l2l_level(const DevicePlan& d, const ShiftOpDev& op, int p, int first, int count, hipStream_t s);
// y[i] += the far field of row i (tree order).  With perm: y_out[perm[i]] = y[i] + the far field instead, y left as it is --
// the result scatter folded into L2P's store (Laplace only; the caller makes sure the L2P groups cover every row)
hipError_t launch_l2p(const DevicePlan& d, int p, double* y, hipStream_t s, const uint32_t* perm = nullptr, double* y_out = nullptr);
// ---- treecode evaluator (FMMBEM_EVAL_TREECODE): the far field by M2P instead of M2L, L2L and L2P ----
// Work of m2p_kernel, built once per geometry.  An item is up to 64 consecutive rows of one target leaf; the leaf's chain is the
// boxes from the root down to the leaf itself that are the target of an M2L pair, and the sources of a chain box are its range of
// DevicePlan::m2l_ptr / m2l_src, in list order.  Leaves whose chain is empty have no item.
struct M2PWork {
  const int *item_leaf = nullptr, *item_row = nullptr;   // [n_items] leaf index, first row of the item within the leaf
  int n_items = 0;
  const int *chain_ptr = nullptr, *chain_box = nullptr;  // [nleaves + 1] -> chain_box
};
// y[i] += (POTENTIAL row) or -= (NORMAL_DERIV row) the sum over the row's chain of M2P(M[source], centre[source], centroid i); Laplace
hipError_t launch_m2p(const DevicePlan& d, const M2PWork& w, int p, double* y, hipStream_t s);
// ---- field quantities (kernels_field.hip; plans over separate targets, whose target rows begin at n_src) ----
// Gradient: Laplace plans, 3 doubles per target row; Pressure (1) and VelocityGradient (9, [k][m]): Stokes field plans whose targets
// are all VELOCITY targets.  tree: width doubles per target row, tree order.
// near: tree[row] = the near pairs' sums, every target row written (zeros where the leaf has no near pair);
// l2p: tree[row] += what the quantity reads of the leaf's local expansions -- + (flag 0) or - (flag 1) the gradient of the row's
//      slot; - (d_x phi_0 + d_y phi_1 + d_z phi_2) of slots 0..2; (1 / 2 mu) [d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3]
//      of slots 0..3 (nothing at p = 1); Hessian: Laplace plans, 9 doubles per target row ([a][b], symmetric), + or - the Hessian of
//      the row's slot (nothing at p = 1);
// scatter: out[width perm[row] ..] = tree[width (row - n_src) ..];
// entries: gamma (3 doubles), pi (3), Gamma (27, [k][m][e]) or eta (9, [a][b]) for pairs laid out as launch_kernel_entries takes them
enum class FieldQuantity { Gradient, Pressure, VelocityGradient, Hessian };
hipError_t launch_near_field(FieldQuantity q, const DevicePlan& d, int64_t n_src, double* tree, hipStream_t s);
hipError_t launch_near_flow(const DevicePlan& d, int64_t n_src, double* q_tree, double* g_tree, hipStream_t s);   // Pressure and VelocityGradient in one kernel
// the representation execute (Laplace): both layers' near pairs in one kernel, sigma in d.xt and mu in mu_tree, phi_tree (1 double
// per target row) and g_tree (3) as above, either null: not computed; M slot 0 += (set: =) M slot 1 at the P2M leaves; the scatter
// of one double per row
hipError_t launch_near_representation(const DevicePlan& d, int64_t n_src, const double* mu_tree, double* phi_tree, double* g_tree, hipStream_t s);
hipError_t launch_fold_slots(const DevicePlan& d, int p, bool set, hipStream_t s);
hipError_t launch_value_scatter(const DevicePlan& d, int64_t n_src, const double* tree, double* out, hipStream_t s);
hipError_t launch_l2p_field(FieldQuantity q, const DevicePlan& d, int p, int64_t n_src, double* tree, hipStream_t s);
hipError_t launch_field_scatter(FieldQuantity q, const DevicePlan& d, int64_t n_src, const double* tree, double* out, hipStream_t s);
hipError_t launch_field_entries(FieldQuantity q, const DevicePlan& d, int m, double* out, hipStream_t s);
hipError_t launch_near_assemble_stokes(const DevicePlan& d, hipStream_t s);
hipError_t launch_p2m_stokes(const DevicePlan& d, int p, hipStream_t s);
hipError_t launch_l2p_stokes(const DevicePlan& d, int p, double* y, hipStream_t s);

// ---- batched execute (fmmbem_plan_execute_batch): one pass over the near matrix / the P2M tables for nv vectors ----
constexpr int kBatchMax = 8;                           // most vectors of one pass
struct BatchVecs {                                     // per vector of the pass: tree-order x and y, its multipole set
  double* xt[kBatchMax];
  double* yt[kBatchMax];
  double2* M[kBatchMax];
  int nv;                                              // vectors of this pass; the kernels may also run slots nv .. width-1 (scratch)
  int width;                                           // slots allocated: 2, 4 or 8 (Stokes: 2, 3 or 4)
};
// the pipelined one-unknown SpMV (near_spmv_pipe_kernel) for nv vectors: bit for bit nv calls of launch_near_spmv; plans where
// launch_near_spmv takes that kernel only (batch_near_ok, launch_choice.hpp)
hipError_t launch_near_spmv_multi(const DevicePlan& d, const BatchVecs& b, hipStream_t s);
// near_spmv_sym3 (Stokes, symmetric blocks) for nv = 2 .. 4 vectors: bit for bit nv calls of launch_near_spmv; the plans it serves
// at a pass of `width` vectors (fmmbem_options.stokes_batch_width; batch_near_sym3_ok, launch_choice.hpp)
hipError_t launch_near_sym3_multi(const DevicePlan& d, const BatchVecs& b, hipStream_t s);
// P2M for nv vectors: the streaming kernel once where launch_p2m streams (one live slot, p >= 8), else launch_p2m per vector
hipError_t launch_p2m_multi(const DevicePlan& d, const BatchVecs& b, int p, hipStream_t s);

// ---- Direct sum (kernels_direct.hip): y_i = sum_j K(t_i, panel j) x_j over ALL of d's panels, m targets ----
int direct_chunk();                                    // FMMBEM_DIRECT_CHUNK: sources per partial sum
int64_t direct_chunks(int64_t n_sources);              // partial sums per target
// point i = (tx, ty, tz)[i * tstride]; tbc null: flags 0; part: direct_chunks(d.n) * m * d.dof doubles of scratch; y: m * d.dof
hipError_t launch_direct(const DevicePlan& d, int64_t m, const double* tx, const double* ty, const double* tz, int tstride,
                         const uint8_t* tbc, const double* x, double* part, double* y, hipStream_t s);
// the field quantities at points: out_i = sum_j (q's pair function)(t_i, panel j) x_j, W = direct_field_width(q) doubles per target
// (3, 1, 9, 9).  pts: m x 3; tbc (Gradient and Hessian only) null: flags 0; x: d.n * d.dof; part: direct_chunks(d.n) * m * W doubles of scratch;
// out: m * W.  Gradient and Hessian take a Laplace d, the other two a Stokes d (hipErrorInvalidValue otherwise).
int direct_field_width(FieldQuantity q);
hipError_t launch_direct_field(FieldQuantity q, const DevicePlan& d, int64_t m, const double* pts, const uint8_t* tbc, const double* x,
                               double* part, double* out, hipStream_t s);


}  // namespace fmmbem
