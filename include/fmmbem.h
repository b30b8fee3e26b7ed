/* fmmbem.h -- C ABI of the MI355X-native FMM-BEM matvec (libfmmbem_hip.so).
 *
 * Drop-in boundary for the reference's hot path
 *     FMM_plan<LaplaceSphericalBEM>::FMM_plan / ::execute / ::kernel().set_p / ::options
 * (reference: include/FMM_plan.hpp:34-43, :75-90, :66-71, :94-96), i.e. everything that
 * include/executor/ExecutorSingleTree.hpp and EvalInteractionLazySparse.hpp do behind it.
 * Plain C types only: pointers, sizes, PODs.  No exit(), no stdout; every entry point returns
 * an fmmbem_status (0 = success) and fmmbem_last_error() gives the text of the last failure on
 * the calling thread.
 *
 * Threading: one in-flight execute per plan (as the reference: a plan is not re-entrant,
 * ExecutorSingleTree.hpp:120-129); distinct plans may run concurrently.
 */
#ifndef FMMBEM_H
#define FMMBEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMMBEM_VERSION 1

/* fmmbem_options is in its second layout: stokes_batch_width was appended and sizeof grew from 120 to 128 bytes.  The six
 * functions that take the struct are therefore bound, through the names below, to entry points that know the 128-byte layout;
 * the library keeps exporting the plain names with the 120-byte layout (the new field taken as 0), so a program compiled against
 * the earlier header runs on this library unchanged -- fmmbem_options_default never writes past the struct its caller holds.
 * Callers that look symbols up by name (dlsym, ctypes) and hold the struct below ask for the _r2 names. */
#define fmmbem_options_default     fmmbem_options_default_r2
#define fmmbem_plan_create         fmmbem_plan_create_r2
#define fmmbem_plan_create_targets fmmbem_plan_create_targets_r2
#define fmmbem_kernel_entries      fmmbem_kernel_entries_r2
#define fmmbem_ops_create          fmmbem_ops_create_r2
#define fmmbem_direct_create       fmmbem_direct_create_r2
#define FMMBEM_PMAX 16          /* expansion orders 1..16 are pre-compiled */

typedef enum {
  FMMBEM_OK = 0,
  FMMBEM_ERR_INVALID = 1,       /* bad argument (null pointer, p out of range, bad quadrature key ...) */
  FMMBEM_ERR_NO_DEVICE = 2,     /* no usable HIP device, or the plan was built host-only            */
  FMMBEM_ERR_HIP = 3,           /* a HIP runtime call or kernel launch failed                         */
  FMMBEM_ERR_ALLOC = 4,         /* host or device allocation failed                                   */
  FMMBEM_ERR_TREE = 5,          /* octree deeper than 21 levels (64-bit Morton keys; the reference's 32-bit keys stop at 10:
                                 * trees that fit 10 levels are built by its rule, bit for bit, deeper ones by the wide coder) */
  FMMBEM_ERR_UNSUPPORTED = 6,   /* option combination not implemented                                 */
  FMMBEM_ERR_IO = 7             /* a mesh file could not be opened or parsed                          */
} fmmbem_status;

/* kernel ids: which reference Kernel class the plan stands in for */
typedef enum {
  FMMBEM_KERNEL_LAPLACE_BEM = 0, /* kernel/LaplaceSphericalBEM.hpp: 1 unknown per panel                  */
  FMMBEM_KERNEL_STOKES_BEM = 1   /* kernel/StokesSphericalBEM.hpp: 3 unknowns per panel, x/y hold Vec<3,double> per panel.
                                  * VELOCITY panels (stokeslet single layer, the operator the solve uses): everything.
                                  * TRACTION panels (bc flag 1, eval_traction_integral :160-258; the TARGET's flag picks the
                                  * operator, :377-389): near-matrix entries, fmmbem_kernel_entries, the near-field evaluators
                                  * (LOCAL, BLOCK_DIAGONAL), and through the FMM evaluator a double-layer far field checked
                                  * against the Direct sum (the reference's own disagrees with its Direct); p_max <= 12 */
} fmmbem_kernel;

/* boundary-condition flag per panel: LaplaceSphericalBEM::Panel::BoundaryType
 * (kernel/LaplaceSphericalBEM.hpp:40) */
enum { FMMBEM_BC_POTENTIAL = 0, FMMBEM_BC_NORMAL_DERIV = 1 };

/* Mirrors FMMOptions (include/FMMOptions.hpp:9-60) + the kernel constructor arguments
 * LaplaceSphericalBEM(p, k) (kernel/LaplaceSphericalBEM.hpp:131) + device placement.
 * Initialise with fmmbem_options_default(). */
/* executor/make_executor.hpp:24-60 (FMMOptions lazy_evaluation / local_evaluation / block_diagonal) */
typedef enum {
  FMMBEM_EVAL_FMM = 0,            /* EvalInteractionLazy(Sparse): near field + far field (the solver's operator)      */
  FMMBEM_EVAL_LOCAL = 1,          /* EvalLocal(Sparse): the near-field blocks only (Preconditioners::LocalInnerSolver,
                                   * examples/BEM/LocalPC.hpp:26-59)                                                  */
  FMMBEM_EVAL_BLOCK_DIAGONAL = 2, /* EvalDiagonalSparse: every leaf with itself (examples/BEM/BlockDiagonalPC.hpp:16-60)  */
  /* 3 is no evaluator and stays FMMBEM_ERR_INVALID (callers probe it as "no such evaluator") */
  FMMBEM_EVAL_TREECODE = 4        /* EvalInteractionLazySparse<Context, false> (FMMOptions::TREECODE, `-eval TREE`): the FMM plan's
                                   * lists, near field and upward pass; every long-range pair (source box, target box) is then
                                   * evaluated by M2P at the bodies of the target box -- no L, L2L or L2P
                                   * (executor/EvalInteractionLazySparse.hpp:269-283).  Laplace, fmmbem_plan_create / _create_like,
                                   * sparse_local 0 or 1, host_only, on one device.  FMMBEM_ERR_UNSUPPORTED: Stokes, shard_world > 1,
                                   * a device list (n_devices > 1 or FMMBEM_DEVICES), fmmbem_plan_create_targets.
                                   * near_stream_fraction is taken as 1 and near_f32_max_p as 0 (accepted without effect), l2l_rule
                                   * has no effect.  fmmbem_plan_get_expansions("L") returns FMMBEM_ERR_UNSUPPORTED: the plan holds
                                   * no local expansions.  fmmbem_stats: the list counts are the FMM plan's (l2p_leaves and l2l_ops as
                                   * built, though nothing runs on them); ms_m2l carries the M2P time, ms_mh, ms_l2l and ms_l2p are 0.
                                   * The same bits on every run, graph replay and batch.                                       */
} fmmbem_evaluator;

/* Downward pass.  The reference's lazy evaluator queues L2L parent->child only for children that were not an M2L
 * target EARLIER in the traversal than the parent (propagate_local / initialised_L,
 * executor/EvalInteractionLazySparse.hpp:199-237): on adaptive trees such a child never receives the far field its
 * ancestors collected and the result carries an error that does not decrease with p.  The reference's sphere meshes
 * produce no such edge, there the two rules are the same list.  fmmbem_stats.l2l_reference_omitted counts them. */
typedef enum {
  FMMBEM_L2L_COMPLETE = 0,        /* every child of a box that holds a local expansion (default)                      */
  FMMBEM_L2L_REFERENCE = 1        /* exactly the reference's list, omissions included (bit parity on adaptive trees)  */
} fmmbem_l2l_rule;

typedef struct {
  int32_t  kernel;            /* fmmbem_kernel                                                     */
  int32_t  p_max;             /* largest expansion order any execute() will ask for (1..16)        */
  int32_t  quad_k;            /* Gauss rule key K: 1,3,4,7,13,17,19,25 (GaussQuadrature.hpp)       */
  double   theta;             /* FMMOptions::set_mac_theta, default 0.5 (FMMOptions.hpp:45)        */
  uint32_t ncrit;             /* FMMOptions::set_max_per_box, default 64 (FMMOptions.hpp:46-47)    */
  int32_t  sparse_local;      /* 1: assembled near matrix (EvalInteractionLazySparse, what the BEM
                               *    drivers select); 0: matrix-free near field recomputed every
                               *    matvec (EvalInteractionLazy, `-disable_sparse`)                  */
  int32_t  host_only;         /* 1: build tree + lists on the host, touch no device (CPU tests)    */
  int32_t  device;            /* HIP device ordinal                                                */
  int32_t  shard_rank;        /* target-leaf shard owned by this plan: rank of world               */
  int32_t  shard_world;       /* 1 = whole operator                                                */
  int32_t  quad_k_fine;       /* Stokes: near-regime Gauss rule K_fine (StokesSphericalBEM::set_Kfine,
                               * kernel/StokesSphericalBEM.hpp:139-141; ctor default 25, driver 19)  */
  int32_t  evaluator;         /* fmmbem_evaluator: which branch of make_evaluators the plan takes   */
  double   mu;                /* Stokes: viscosity (StokesSphericalBEM(p,k,mu), :131)               */
  int32_t  shard_upward;      /* shard_world > 1: also shard P2M/M2M by owner; the multipoles are exchanged by ONE
                               * collective the caller performs between fmmbem_plan_upward_device and
                               * fmmbem_plan_downward_device: 1 = an all-gather of every shard's multipoles, 2 = an
                               * all-to-all of the ones each receiver reads (fmmbem_plan_exchange_counts);
                               * 0: every shard repeats the whole upward pass                                  */
  int32_t  l2l_rule;          /* fmmbem_l2l_rule: which parent->child L2L edges the downward pass applies              */
  double   near_stream_fraction; /* sparse_local = 1: share of the near-field pairs whose entries are STORED and streamed every
                               * matvec (P2P_Lazy::to_matrix + Matvec<>, EvalP2P.hpp:47-98, Matvec.hpp:14-33).  1.0 (default): all
                               * of them, the reference's assembled matrix.  0 <= f < 1, HYBRID: the target leaves with the most
                               * rows keep no matrix until they hold 1 - f of the pairs; their far-regime entries are recomputed
                               * every matvec from the quadrature points (what EvalInteractionLazy::eval_P2P_lists does,
                               * EvalInteractionLazy.hpp:239-252) by the SAME kernel between its streamed items -- arithmetic in
                               * the issue slots the HBM-bound stream leaves empty -- and their near-regime entries are evaluated
                               * once.  Footprint and HBM bytes fall by 1 - f; a row's sum is formed in a fixed order, results
                               * differ from f = 1 in the last bits.  Taken as 1 where the hybrid kernel does not apply (rules of
                               * more than 3 / 4 points, the LOCAL / BLOCK_DIAGONAL evaluators).  FMMBEM_NEAR_STREAM_FRACTION
                               * overrides it at creation (sweeps).                                                      */
  int32_t  n_devices;         /* > 1: ONE plan over the devices listed in `devices` (at most 8; SURVEY 8b "device list"): the target leaves
                               * are sharded over them inside the handle, which copies x to every device, exchanges the multipoles
                               * the shards' lists read and brings the result slices home by peer copies over xGMI; x and y of
                               * fmmbem_plan_execute_device / fmmbem_gmres_device live on devices[0].  The same bits as one device.
                               * shard_upward = 0 then makes every device repeat the upward pass instead of exchanging multipoles.
                               * 0 or 1: the single `device`.  With n_devices == 0 the environment variable FMMBEM_DEVICES=0,1,...
                               * supplies a list (for callers that cannot: the reference's unmodified drivers)                  */
  int32_t  devices[8];
  int32_t  near_f32_max_p;    /* Float near field.  0 (default): off.  1..16: an execute at an order p <= this value streams a copy
                               * of the assembled near matrix rounded to float (half the bytes of the pass that bounds a low-order
                               * matvec); x, the accumulators and y stay doubles, executes above it run the FP64 kernels on the
                               * FP64 matrix, which is always kept.  Against the FP64 pass row i of the result moves by at most
                               * 2^-24 (|A_near| |x|)_i -- far below the truncation error of the far field at low orders
                               * (DESIGN.md section 8 "Float near field" gives the recommended threshold); the same bits every run.
                               * Active on assembled plans (sparse_local = 1) that are not hybrid, on one device with
                               * shard_world = 1: fmmbem_plan_create / _create_like, every evaluator, Laplace and Stokes with the
                               * symmetric blocks.  Accepted without effect elsewhere (target, matrix-free, hybrid, device-list,
                               * sharded, host-only plans; FMM plans with no M2L pair at all -- every leaf near every other, a few
                               * hundred panels: exact at every order, no truncation error for the rounding to hide under): fmmbem_stats.near_f32_bytes is then 0.  On an active plan
                               * fmmbem_plan_batch_width is 1.  Outside 0..16: FMMBEM_ERR_INVALID.                          */
  int32_t  stokes_batch_width;/* Multi-vector near field of a Stokes plan.  0 or 1 (default 0): off, a batch runs its vectors one after
                               * another.  2, 3, 4: one pass over the near matrix serves that many vectors of
                               * fmmbem_plan_execute_batch(_device) and of the lockstep fmmbem_gmres_batch(_device) -- the matrix is
                               * two thirds of a Stokes matvec and does not depend on the vector; fmmbem_plan_batch_width returns the
                               * value.  Every result stays bit for bit that vector's single execute; the far field runs per vector.
                               * Per slot the plan then keeps x and y in tree order and one multipole set, allocated at the first
                               * batch call.  Active on Stokes plans (VELOCITY, TRACTION or mixed targets; the FMM, LOCAL and
                               * BLOCK_DIAGONAL evaluators) with the assembled near field in symmetric blocks, not hybrid, the float
                               * near field not active, on one device with shard_world = 1; fmmbem_plan_create_like inherits it from
                               * its base.  Accepted without effect elsewhere (Laplace, hybrid, matrix-free, device-list, sharded,
                               * host-only plans, plans with the float copy): the width stays what it was.  The field is appended:
                               * sizeof(fmmbem_options) grows by 8 (the _r2 names above).  Outside 0..4: FMMBEM_ERR_INVALID.
                               * DESIGN.md section 8 "Stokes batched near field" has the measured times per width.               */
} fmmbem_options;

/* Statistics of a plan and of its last execute (times in milliseconds, device-side HIP events). */
typedef struct {
  int64_t n_panels, n_boxes, n_leaves, n_levels;
  int64_t near_nnz;             /* entries of the assembled near matrix owned by this shard          */
  int64_t near_nnz_total;       /* ... of the whole operator                                         */
  int64_t p2p_pairs, m2l_pairs, m2l_pairs_owned, m2m_ops, l2l_ops, p2m_leaves, l2p_leaves;
  int64_t m2l_classes;          /* distinct M2L translation vectors                                  */
  int64_t owned_leaf_begin, owned_leaf_end, owned_row_begin, owned_row_end;
  int64_t near_bytes;           /* HBM bytes of the near-matrix values                               */
  int32_t expansions_active;    /* bit 0: G expansion, bit 1: dG/dn expansion                        */
  int32_t last_p;
  double  build_host_ms, build_assemble_ms;
  /* per-stage device times: MEAN over the executes recorded since timing was (re)enabled */
  double  ms_total, ms_gather, ms_near, ms_scatter, ms_p2m, ms_m2m, ms_mh, ms_m2l, ms_l2l, ms_l2p;
  /* (a fast-path pass of fmmbem_plan_execute_batch records ms_near and ms_p2m only -- on a Stokes plan with stokes_batch_width
   * ms_near only: its P2M runs per vector, unrecorded; where L2P's last store delivers the result -- a Laplace plan on its own
   * panels, one shard, every row under an L2P leaf -- ms_scatter brackets no kernel and ms_l2p includes the delivery) */
  int64_t timed_executes;       /* how many executes the means cover                                 */
  int64_t l2l_reference_omitted;/* L2L edges FMMBEM_L2L_REFERENCE leaves out of this tree (0: the rules coincide) */
  int64_t m2l_items, m2l_passes;/* rotation M2L: work items (one wavefront each) and 64-pair passes over them; pairs / (64 passes)
                                 * is the lane fill                                                   */
  int64_t near_side_entries;    /* matrix-free plans (sparse_local = 0): near-regime pairs evaluated once at creation and kept
                                 * (12 bytes each: column + value); 0 for assembled plans                */
  int32_t m2l_kernel;           /* the M2L an execute at last_p took: 1 rotation kernel, 2 double sum, 3 double sum (lanes = sources),
                                 * 4 M2P (treecode) */
  int32_t expansion_slots;             /* slots per box in M and L (fmmbem_plan_get_expansions): Laplace 2, Stokes 8, 11 with TRACTION targets */
  int64_t rot_nop_orders;       /* build record: orders p of the rotation kernels that were compiled with a wait state in front of
                                 * every DPP FMA because the build's ISA check found the DPP hazard in their code (csrc/Makefile,
                                 * tools/check_rot_isa.py): bit p-1 M2L, bit 16+p-1 M2M, bit 32+p-1 L2L.
                                 * 0 on the toolchain this was developed with; such an order runs ~30 % slower, not wrong */
  int32_t tree_coder_levels;    /* 10: the reference's 32-bit Morton coder built the tree; 21: the 64-bit coder had to (deeper tree) */
  int32_t n_devices;            /* devices this plan runs on (fmmbem_options.n_devices / FMMBEM_DEVICES); the figures above are then the whole
                                 * operator's: owned counts summed over the shards, stage times the longest shard's                    */
  int32_t geometry_shared;      /* plans alive that share this plan's tree, lists and tables (fmmbem_plan_create_like), itself included */
  int64_t near_recomputed_pairs;/* hybrid plans (near_stream_fraction < 1): panel pairs of this shard that are recomputed every matvec
                                 * instead of stored (near_nnz counts all of the shard's entries, near_bytes what is stored)         */
  int64_t near_f32_bytes;       /* HBM bytes of the float copy of the near matrix (fmmbem_options.near_f32_max_p); 0: the float near
                                 * field is not active on this plan                                                                */
  int32_t last_near_f32;        /* 1: the last execute streamed the float copy; after fmmbem_plan_execute_flow: 2 or 3, see there   */
} fmmbem_stats;

typedef struct fmmbem_plan fmmbem_plan;

/* ---- lifecycle -------------------------------------------------------------------------- */
void fmmbem_options_default(fmmbem_options *opts);

/* FMM_plan(const Kernel&, const std::vector<source_type>&, FMMOptions&)  (FMM_plan.hpp:34-43).
 * vertices: n_panels x 3 vertices x 3 coordinates (the arguments of Panel(p0,p1,p2),
 * LaplaceSphericalBEM.hpp:64); bc: n_panels flags or NULL (all POTENTIAL).
 * Builds octree + interaction lists on the host, uploads them once, assembles the near matrix
 * on the device. */
int fmmbem_plan_create(const fmmbem_options *opts, size_t n_panels, const double *vertices,
                       const uint8_t *bc, fmmbem_plan **out);
/* A plan of the SAME panels, options and order as `base` with other boundary-condition flags -- the drivers' right-hand-side plan
 * (examples/LaplaceBEM.cpp:218-232: the panels with their flags switched; StokesBEM.cpp:266-270) and the preconditioners' plans.
 * Tree, permutation, pair lists, work items and operator tables are SHARED with base through a reference count (either plan may
 * be destroyed first); only what the flags decide is built: the near-matrix values, the P2M moments, the expansions.  0.05 s
 * instead of 0.28 s at N = 1M.  fmmbem_plan_create does the same on its own when it is handed the vertices and options of a live
 * plan (recognised by two 64-bit hashes of the vertex bytes; FMMBEM_PLAN_SHARE=0 disables that). */
int fmmbem_plan_create_like(const fmmbem_plan *base, const uint8_t *bc, fmmbem_plan **out);
/* FMM_plan(const Kernel&, const std::vector<source_type>&, const std::vector<target_type>&, FMMOptions&)  (FMM_plan.hpp:45-55):
 * a plan whose targets are POINTS of their own.  An execute computes y_i = sum_j K(t_i, s_j) x_j, K of
 * LaplaceSphericalBEM::operator() (kernel/LaplaceSphericalBEM.hpp:273-297): the target's flag picks the integral of G or of
 * dG/dn over the source panel (its normal), whatever the panels' flags -- what Direct::matvec(K, panels, x, targets) computes
 * (the exterior potential of the drivers, examples/LaplaceBEM.cpp:346-369).  target_points: n_targets x 3; target_bc: n_targets
 * flags or NULL (all POTENTIAL); bc (the panels' flags) does not enter and may be NULL.  Coincident targets are legal.
 * x of fmmbem_plan_execute / _execute_device has n_panels entries, y n_targets, both in the caller's order.
 * Laplace, the FMM evaluator, sparse_local = 1, shard_world = 1, one device and l2l_rule COMPLETE only (FMMBEM_ERR_UNSUPPORTED
 * otherwise); near_stream_fraction is taken as 1.  fmmbem_plan_set_timing, _stats (the SOURCE tree's figures), _get_perm (the
 * panels' permutation), _get_boxes (the source tree), _get_pairs (source box, target box: each in its own tree's numbering),
 * _set_graphs and _destroy take the handle; the calls of whole operators (GMRES, create_like, the sharded and slice calls,
 * near_split, get_near_row, get_diagonal, get_expansions) return FMMBEM_ERR_UNSUPPORTED and leave it usable. */
int fmmbem_plan_create_targets(const fmmbem_options *opts, size_t n_panels, const double *vertices, const uint8_t *bc,
                               size_t n_targets, const double *target_points, const uint8_t *target_bc, fmmbem_plan **out);
typedef struct {
  int64_t n_panels, n_targets;
  int64_t n_target_points;          /* distinct (point, flag) pairs: the bodies of the target tree                      */
  int64_t n_source_boxes, n_source_leaves, n_source_levels;
  int64_t n_target_boxes, n_target_leaves, n_target_levels;
  int32_t tree_coder_levels;        /* 10 or 21, the same for both trees                                                */
  int32_t reserved;
} fmmbem_target_info;
int fmmbem_plan_target_info(const fmmbem_plan *plan, fmmbem_target_info *out);
/* The target tree's boxes in its BFS order (as fmmbem_plan_get_boxes; bodies = target-tree positions of the distinct points) */
int fmmbem_plan_get_target_boxes(const fmmbem_plan *plan, double *center, double *side, int32_t *level, int32_t *is_leaf,
                                 int32_t *parent, int32_t *body_begin, int32_t *body_end);
/* tree_to_point: n_target_points, target-tree position -> distinct point; target_to_point: n_targets, given target -> distinct
 * point.  Either may be NULL. */
int fmmbem_plan_get_target_perm(const fmmbem_plan *plan, uint32_t *tree_to_point, uint32_t *target_to_point);
/* The FIELD PLAN: the field of a layer on the panels at points of their own,
 *   y_i = sum_j K(t_i, s_j) x_j,  K = Kernel::operator()(target, source),
 * for either kernel.  The TARGET's flag picks the operator; the source's normal enters, the panels' own flags do not (there is
 * no bc argument).  target_points: n_targets x 3; target_bc: n_targets flags or NULL (all 0).
 *   FMMBEM_KERNEL_LAPLACE_BEM: the plan of fmmbem_plan_create_targets(opts, n, v, NULL, m, pts, flags) -- one code path, the same
 *     bits in every result.
 *   FMMBEM_KERNEL_STOKES_BEM: x is n_panels x 3, y n_targets x 3, interleaved, in the caller's order.  Flag 0 (VELOCITY): the single
 *     layer, eval_velocity_integral with 1/(2 mu) (kernel/StokesSphericalBEM.hpp:260-375), the four potentials of the far field.
 *     Flag 1 (TRACTION): the double layer, eval_traction_integral (:160-258), the seven dipole potentials.  The live expansion
 *     groups follow the targets' flags alone (8 slots without TRACTION targets, 11 with them); every source feeds every live
 *     group.  The kernels are the single Stokes plan's: a target on a panel's centroid gets that plan's row, bit for bit.
 * Coincident targets (same point, same flag) are one body of the target tree; the result goes back to every copy.
 * Options as fmmbem_plan_create_targets: the FMM evaluator, sparse_local = 1, shard_world = 1, one device, l2l_rule COMPLETE
 * (FMMBEM_ERR_UNSUPPORTED otherwise, as for an unknown kernel id); near_stream_fraction is taken as 1; near_f32_max_p and
 * stokes_batch_width are accepted without effect (fmmbem_plan_batch_width is 1 on a Stokes field plan: a batch runs vector by
 * vector, bit for bit the single executes).  host_only = 1 builds the lists; executing such a plan returns FMMBEM_ERR_UNSUPPORTED.
 * The handle is a plan over separate targets in every respect: fmmbem_plan_target_info, _get_target_boxes, _get_target_perm,
 * _get_perm, _get_boxes, _get_pairs, _stats, _set_timing, _set_graphs, _execute(_device) and _execute_batch(_device) take it as they
 * take the handle of fmmbem_plan_create_targets; the calls of whole operators return FMMBEM_ERR_UNSUPPORTED and leave it usable. */
int fmmbem_plan_create_field(const fmmbem_options *opts, size_t n_panels, const double *vertices, size_t n_targets,
                             const double *target_points, const uint8_t *target_bc, fmmbem_plan **out);
void fmmbem_plan_destroy(fmmbem_plan *plan);

/* ---- the hot path ----------------------------------------------------------------------- */
/* results = plan.execute(charges) with kernel().set_p(p) applied first
 * (FMM_plan.hpp:75-90; GMRES.hpp:194-201).  x, y: n_panels x dof doubles (dof = 1 Laplace, 3 Stokes,
 * interleaved per panel as std::vector<Vec<3,double>>) in ORIGINAL panel order, HOST pointers; y is overwritten.  With shard_world > 1, y holds this shard's rows and zeros
 * elsewhere (sum over shards = full result). */
int fmmbem_plan_execute(fmmbem_plan *plan, int p, const double *x, double *y);

/* Optional, for callers that keep their vectors: page-lock a host buffer (hipHostRegister) so that the two copies of a
 * host-pointer execute run at the PCIe rate instead of through the runtime's staging of pageable memory (INTEGRATION.md gives
 * the measured difference).  The caller owns the memory: unregister BEFORE freeing or reallocating it -- which is why the
 * library never registers a caller's pointer on its own (a std::vector that the reference's solver reallocates would leave a
 * stale registration behind).  Not needed for fmmbem_gmres, whose vectors cross PCIe once per solve. */
int fmmbem_host_register(void *ptr, size_t bytes);
int fmmbem_host_unregister(void *ptr);

/* Same, with DEVICE pointers and an explicit hipStream_t (NULL = default stream); asynchronous. */
int fmmbem_plan_execute_device(fmmbem_plan *plan, int p, const double *d_x, double *d_y, void *stream);

/* Near-field part only: y = A_near x (what Matvec<> does in EvalInteractionLazySparse.hpp:136-148).
 * DEVICE pointers, asynchronous. */
int fmmbem_plan_near_device(fmmbem_plan *plan, const double *d_x, double *d_y, void *stream);

/* Batched execute: k vectors on one plan at order p, each result bit for bit what fmmbem_plan_execute(_device) gives for that
 * vector.  Vector j is x + j*ldx (n_panels x dof doubles, caller's panel order), result j is y + j*ldy (n_panels x dof doubles,
 * or n_targets for a target plan); the doubles between vectors are neither read nor written.  k < 1, a null pointer or a
 * leading dimension shorter than the vector give FMMBEM_ERR_INVALID; everything else is refused as execute refuses it (a
 * host-only plan FMMBEM_ERR_NO_DEVICE, a host-only target plan FMMBEM_ERR_UNSUPPORTED, the host form with result slices
 * FMMBEM_ERR_INVALID).  Any k: the call works through it in passes of at most fmmbem_plan_batch_width vectors.
 * Fast path -- Laplace plans, assembled (sparse_local = 1), not hybrid (a plan whose near_stream_fraction < 1 fell back to the
 * streamed matrix counts as not hybrid), one device, shard_world = 1, no result slices; single, create_like and target plans;
 * the FMM, LOCAL and BLOCK_DIAGONAL evaluators: one pass over the near-field matrix serves every vector of the pass (and one
 * pass over the P2M tables, where a single execute streams them: one live slot, p >= 8); M2M, M2L, L2L, L2P, the gather and
 * the delivery run once per vector.  Stokes plans created with fmmbem_options.stokes_batch_width = 2, 3 or 4 (see there for the
 * plans it is active on) take the same path with near_spmv_sym3 for that many vectors; P2M, like the rest of the far field, runs
 * per vector.  Every other plan (Stokes without that option, hybrid, matrix-free, device lists, shard_world > 1, result
 * slices) runs the k vectors one after another inside the call.
 * Batch buffers (per vector of a pass: x and y in tree order, one multipole set) are allocated on the plan's device at the
 * first batch call and kept until destroy; if that fails the call returns FMMBEM_ERR_ALLOC and single executes still work.
 * Batches never capture or replay graphs, whatever fmmbem_plan_set_graphs says.  With stage timing on, a fast-path pass records
 * its near-field and P2M passes only (fmmbem_plan_stats: ms_near, ms_p2m per pass; a Stokes pass its near-field pass alone:
 * its P2M runs per vector and is not recorded, ms_p2m then covers no batch work); a batch run vector by vector records as
 * its single executes do.
 * The host form takes HOST pointers and returns when y is written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_batch(fmmbem_plan *plan, int p, int k, const double *x, size_t ldx, double *y, size_t ldy);
int fmmbem_plan_execute_batch_device(fmmbem_plan *plan, int p, int k, const double *d_x, size_t ldx,
                                     double *d_y, size_t ldy, void *stream);
/* Vectors one pass of the near field serves on this plan: > 1 on the fast path above, 1 where the batch runs vector by vector
 * (also on a host-only plan). */
int fmmbem_plan_batch_width(const fmmbem_plan *plan, int *width);

/* ---- Field gradient: the gradient of the Laplace field at the points of a plan over separate targets ----------------------
 * (no reference counterpart: the electric field, the velocity of a potential flow, the flux are -grad phi off the surface).
 * On a Laplace plan of fmmbem_plan_create_targets or fmmbem_plan_create_field, for target i with point t_i,
 *   g_i = sum_j gamma(t_i, s_j) x_j,   three doubles,
 * gamma = the gradient WITH RESPECT TO THE TARGET POINT of the integrand the target's flag picks.  The rule is chosen as
 * eval_dGdn chooses it for a NORMAL_DERIV target (kernel/LaplaceSphericalBEM.hpp:208-264): dist = |t - c_j|;
 * nearby = sqrt(2 A_j) / dist >= 0.5; the 16-point rule on the vertices if nearby, else the K stored points.  With dx = y_q - t:
 *   flag 0 (gradient of the single layer, int G):        gamma = sum_q w_q A_j dx / |dx|^3;  dist < 1e-8: gamma = 2 pi n_j, the
 *     reference's self value of the derivative kernel -- so n_j . gamma(t, s_j) is, for every pair and regime, the entry K(t, s_j)
 *     of a NORMAL_DERIV target;
 *   flag 1 (gradient of the double layer, int dG/dn_y):  gamma = sum_q w_q A_j (-n_j / |dx|^3 + 3 (dx . n_j) dx / |dx|^5);
 *     dist < 1e-8: gamma = 0.
 * n_j is the panel normal as the plan holds it.  The far field is +- grad of the local expansion that the potential execute
 * evaluates: the slot picked by the target's flag, + for flag 0 and - for flag 1, as its L2P adds the value.  The gradient of the
 * representation formula is (g[flag 0 plan, density] - g[flag 1 plan, potential]) / (4 pi).
 * x: n_panels doubles; g: n_targets x 3, interleaved, both in the caller's order; coincident targets each get their copy.
 * The execute is the potential execute's gather, P2M, M2M, M2L and L2L, then two kernels of its own -- the near pairs matrix-free
 * (a row's sum: the leaf's near list in order, panels ascending, quadrature points in order) and the gradient of L (terms
 * m-major) -- and the delivery: the same bits every run.  Its buffers are allocated at the first gradient call
 * (FMMBEM_ERR_ALLOC if that fails; the plan stays usable).  Checked in this order: a null plan or vector -> FMMBEM_ERR_INVALID;
 * p outside 1..p_max -> _INVALID; a plan that is not over separate targets -> _UNSUPPORTED; a Stokes plan -> _UNSUPPORTED; a
 * host-only plan -> _UNSUPPORTED; the handle stays usable.  A gradient execute is launched plainly, kernel by kernel, whatever
 * fmmbem_plan_set_graphs says, and leaves the captured graphs of the potential execute as they are.  With stage timing on it is
 * recorded as an execute: ms_near is the near kernel of the gradient, ms_l2p the gradient of L.  No batches.
 * The host form takes HOST pointers and returns when g is written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_gradient(fmmbem_plan *plan, int p, const double *x, double *g);
int fmmbem_plan_execute_gradient_device(fmmbem_plan *plan, int p, const double *d_x, double *d_g, void *stream);

/* ---- Field Hessian: the second derivatives of the Laplace field at the points of a plan over separate targets -------------
 * (no reference counterpart: the strain rate of a potential flow, the field gradient in the force on a dipole, the tidal tensor, a
 * second-order Taylor step, Newton's method for stagnation points).  On a Laplace plan of fmmbem_plan_create_targets or
 * fmmbem_plan_create_field, for target i with point t_i,
 *   H_i[a][b] = sum_j eta_ab(t_i, s_j) x_j,   nine doubles, row-major,
 * eta_ab = d gamma_a / d t_b, the derivative WITH RESPECT TO THE TARGET POINT of the entry gamma of the field gradient above for the
 * target's flag: H is the matrix of second derivatives of what fmmbem_plan_execute returns at that point.  The rule is chosen
 * exactly as for gamma, by the same expressions, so that a pair is in the same regime in both: dist = |t - c_j|;
 *   dist < 1e-8: eta = 0 for both flags (the second derivative jumps across the layer; a point on it is the caller's business, as
 *     for the Stokes quantities);
 *   sqrt(2 A_j) / dist >= 0.5: the 16-point rule on the vertices;  otherwise the K stored points.
 * With dx = y_q - t, r = |dx| and n the panel normal as the plan holds it:
 *   flag 0 (single layer):  eta_ab = sum_q w_q A_j ( 3 dx_a dx_b / r^5 - delta_ab / r^3 )
 *   flag 1 (double layer):  eta_ab = sum_q w_q A_j ( 15 (dx.n) dx_a dx_b / r^7 - 3 (n_a dx_b + n_b dx_a + (dx.n) delta_ab) / r^5 )
 * Both are symmetric and trace-free point by point.  The far field is +- the Hessian of the local expansion of the slot the
 * target's flag picks, + for flag 0 and - for flag 1: the exact Hessian of the truncated expansion, evaluated as the Cartesian
 * gradients of the three expansions of order p - 1 that d_x phi, d_y phi, d_z phi are.  At p = 1 and p = 2 that expansion has no
 * second derivative and the result is the near half.
 * The upper triangle is computed and the lower mirrors it: H[a][b] and H[b][a] carry the same bits.  The trace is left as computed,
 * zero to rounding, not forced.  The physical Hessian of the representation formula is
 * (H[flag 0 plan, density] - H[flag 1 plan, potential]) / (4 pi).
 * x: n_panels doubles; H: n_targets x 9, both in the caller's order; coincident targets each get their copy.  The execute is the
 * gradient execute's with its own two kernels -- the near pairs matrix-free (a row's sums: the leaf's near list in order, panels
 * ascending, quadrature points in order) and the Hessian of L (terms m-major) --: the same bits every run.  Its buffers are
 * allocated at the first Hessian call (FMMBEM_ERR_ALLOC if that fails; the plan stays usable).  Checked in the gradient's order:
 * a null plan or vector -> FMMBEM_ERR_INVALID; p outside 1..p_max -> _INVALID; a plan that is not over separate targets ->
 * _UNSUPPORTED; a Stokes plan -> _UNSUPPORTED; a host-only plan -> _UNSUPPORTED; the handle stays usable and no pointer is
 * touched.  Launched plainly, whatever fmmbem_plan_set_graphs says; the captured graphs of the potential execute stay as they are.
 * Stage timing: ms_near is its near kernel, ms_l2p the Hessian of L (0 at p = 1, where it is not launched).  No batches.  The Hessian
 * on the plan's own panels is not built.
 * The host form takes HOST pointers and returns when H is written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_hessian(fmmbem_plan *plan, int p, const double *x, double *H);
int fmmbem_plan_execute_hessian_device(fmmbem_plan *plan, int p, const double *d_x, double *d_H, void *stream);

/* ---- Field pressure: the pressure of the Stokes single layer at the points of a field plan ----------------------------------
 * (no reference counterpart: the other half of a Stokes field off the surface).  On a Stokes plan of fmmbem_plan_create_field
 * whose targets are all VELOCITY targets, for target i with point t_i,
 *   q_i = sum_j pi(t_i, s_j) . x_j,   one double;  x_j the 3 components of panel j,
 *   pi(t, s_j) = sum_q w_q A_j d_q / |d_q|^3,   d_q = t - y_q.
 * Scaling: the plan's execute returns u' = (1/2mu) int (I/r + d d^T/r^3) f dS = 4 pi u; q is the pressure that belongs to that
 * u': -grad q + mu lap u' = 0 off the surface.  The physical pressure is q / (4 pi), as the physical velocity is u' / (4 pi); there
 * is no mu in pi.
 * The rule is chosen as the velocity entry chooses it: dist = |t - c_j|; dist < 1e-8: pi = 0 -- the mean of the two one-sided
 * limits +-2 pi n_j of a flat panel, with the in-plane part of its own integral neglected: the pressure jumps across the layer,
 * and a point ON it is the caller's business; otherwise sqrt(2 A_j) / dist >= 0.5: the K_fine rule on the vertices; otherwise
 * the K stored points.  A quadrature point with |d_q|^2 < 1e-8 contributes 0.
 * The far field: q_i -= d_x phi_0 + d_y phi_1 + d_z phi_2 at t_i, phi_k the local expansion of the potential with charges f_k
 * that the velocity execute holds after L2L (slot k of the leaf; unscaled: the 1/(2 mu) of the velocity's L2P does not enter;
 * slot 3 is not read).  In the far regime, with the same K, pi is minus the flag-0 gamma of the field gradient above.
 * x: n_panels x 3 doubles; q: n_targets doubles, both in the caller's order; coincident targets each get their copy.
 * The execute is the velocity execute's gather, P2M, M2M, M2L and L2L, then two kernels of its own -- the near pairs matrix-free
 * (a row's sum: the leaf's near list in order, panels ascending, quadrature points in order) and minus the divergence of the
 * three expansions (terms m-major) -- and the delivery: the same bits every run.  Its buffers are allocated at the first pressure
 * call (FMMBEM_ERR_ALLOC if that fails; the plan stays usable).  Checked in this order: a null plan or vector ->
 * FMMBEM_ERR_INVALID; p outside 1..p_max -> _INVALID; a plan that is not over separate targets -> _UNSUPPORTED; a Laplace plan ->
 * _UNSUPPORTED; a plan with any TRACTION target -> _UNSUPPORTED; a host-only plan -> _UNSUPPORTED; the handle stays usable and
 * neither pointer is touched.  A pressure execute is launched plainly, kernel by kernel, whatever fmmbem_plan_set_graphs says,
 * and leaves the captured graphs of the velocity execute as they are.  With stage timing on it is recorded as an execute:
 * ms_near is the near kernel of the pressure, ms_l2p the divergence of L.  No batches.
 * The host form takes HOST pointers and returns when q is written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_pressure(fmmbem_plan *plan, int p, const double *x /* n x 3 */, double *q /* n_targets */);
int fmmbem_plan_execute_pressure_device(fmmbem_plan *plan, int p, const double *d_x, double *d_q, void *stream);

/* ---- Field velocity gradient: the gradient of the Stokes single layer's velocity at the points of a field plan ---------------
 * (no reference counterpart: with the pressure above it gives the stress sigma = -p I + mu (grad u + grad u^T) off the surface).
 * On a Stokes plan of fmmbem_plan_create_field whose targets are all VELOCITY targets, for target i with point t_i,
 *   G_i[k][m] = d u'_k / d t_m,   nine doubles, row-major,
 * u' what the plan's execute returns there: u' = (1/2mu) int (I/r + d d^T/r^3) f dS = 4 pi u.  The scaling is execute's, the
 * 1/(2 mu) included; the physical gradient is G / (4 pi).
 * Near pairs: with d = t - y_q and s = d . f_j,
 *   G[k][m] += (1/2mu) sum_q w_q A_j [ (-f_k d_m + delta_km s + d_k f_m) / r^3 - 3 s d_k d_m / r^5 ].
 * The rule is chosen as the pressure chooses it: dist = |t - c_j|; dist < 1e-8: the pair contributes 0 -- the gradient jumps
 * across the layer, and a point ON it is the caller's business; otherwise sqrt(2 A_j) / dist >= 0.5: the K_fine rule on the
 * vertices; otherwise the K stored points.  A quadrature point with |d_q|^2 < 1e-8 contributes 0.
 * The far field: with phi_0..phi_3 the four local expansions of the leaf after L2L and x the target's own coordinates,
 *   G[k][m] += (1/2mu) [ d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3 ].
 * The second derivatives are first derivatives of the expansions of order p - 1 that d_x phi, d_y phi, d_z phi are, their
 * coefficients linear in L: no second derivative by the spherical chain rule, one division by sin(alpha) per row.  An order p
 * execute has the Hessian terms of degrees below p - 1 only: at p = 1 the far half is 0, at p = 2 only its antisymmetric part is
 * not.  Both halves are trace-free term by term (every quadrature point's tensor, every R_nm harmonic): G[0][0] + G[1][1] +
 * G[2][2] is rounding-level.
 * x: n_panels x 3 doubles; G: n_targets x 9 doubles, both in the caller's order; coincident targets each get their copy.
 * The execute is the velocity execute's gather, P2M, M2M, M2L and L2L, then two kernels of its own -- the near pairs matrix-free
 * (a row's nine sums: the leaf's near list in order, panels ascending, quadrature points in order) and the far field above (terms
 * m-major) -- and the delivery: the same bits every run.  Its buffers are allocated at the first call (FMMBEM_ERR_ALLOC if that
 * fails; the plan stays usable).  Checked in this order: a null plan or vector -> FMMBEM_ERR_INVALID; p outside 1..p_max ->
 * _INVALID; a plan that is not over separate targets -> _UNSUPPORTED; a Laplace plan -> _UNSUPPORTED; a plan with any TRACTION
 * target -> _UNSUPPORTED; a host-only plan -> _UNSUPPORTED; the handle stays usable and neither pointer is touched.  It is
 * launched plainly, kernel by kernel, whatever fmmbem_plan_set_graphs says, and leaves the captured graphs of the velocity
 * execute as they are.  With stage timing on it is recorded as an execute: ms_near is the near kernel of the gradient, ms_l2p its
 * far-field kernel.  No batches.  fmmbem_plan_execute_gradient goes on refusing Stokes plans.
 * The host form takes HOST pointers and returns when G is written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_velocity_gradient(fmmbem_plan *plan, int p, const double *x /* n x 3 */, double *G /* n_targets x 9 */);
int fmmbem_plan_execute_velocity_gradient_device(fmmbem_plan *plan, int p, const double *d_x, double *d_G, void *stream);

/* ---- Flow execute: velocity, pressure and velocity gradient at the points of a field plan in one pass ------------------------
 * (no reference counterpart).  On a Stokes plan of fmmbem_plan_create_field whose targets are all VELOCITY targets, each non-null
 * output is BIT FOR BIT what fmmbem_plan_execute (u), fmmbem_plan_execute_pressure (q) and fmmbem_plan_execute_velocity_gradient
 * (G) write for the same plan, p and x -- the caller's order and coincident targets included.  A null output is not computed.
 * One call is one gather, one P2M and one far chain through L2L, where the single executes run one each; then, per output asked,
 * the kernels its single execute launches, on the same L:
 *   u       the stored near matrix by the plan's near SpMV into the tree-order result (target rows zero-filled first, as
 *           execute does it), the velocity's L2P, the delivery;
 *   q or G  alone: that quantity's matrix-free near kernel and its L2P kernel;
 *   q and G ONE near kernel for both -- one walk over a row's near lists, a panel's record staged once, one regime test per
 *           pair, one t - y_q, |d_q|^2 and reciprocal square root per quadrature point feeding both quantities' updates, a row's
 *           ten sums in the list order of the single kernels -- then the pressure's and the gradient's L2P kernels as they stand.
 * The pressure's and the gradient's buffers are those of their single executes, allocated at first use (FMMBEM_ERR_ALLOC if that
 * fails; the plan stays usable).  Launched plainly, kernel by kernel, whatever fmmbem_plan_set_graphs says; the captured graphs
 * of execute are left as they are, and execute, execute_batch and the single field executes return the same bits before and
 * after a flow execute.
 * Checked in this order: a null plan -> FMMBEM_ERR_INVALID; a null x, or u, q and G all null -> _INVALID; p outside 1..p_max ->
 * _INVALID; a plan that is not over separate targets -> _UNSUPPORTED; a Laplace plan -> _UNSUPPORTED; a plan with any TRACTION
 * target -> _UNSUPPORTED, whichever outputs are asked; a host-only plan -> _UNSUPPORTED.  A refusal touches no pointer and leaves
 * the handle usable.
 * With stage timing on a flow execute is recorded as ONE execute: ms_near brackets all its near work (the SpMV of u and the near
 * kernel(s) of q and G), ms_l2p all its L2P kernels, the other stages as in a field execute.  fmmbem_stats.last_near_f32 after a
 * flow execute says which near path q and G took: 2 the one kernel for both, 3 a single quantity's kernel, 0 neither was asked
 * (an execute sets it back to 0 or 1).  No TRACTION targets, no batches, no graphs, no shards.
 * x: n_panels x 3 doubles; u: n_targets x 3, q: n_targets, G: n_targets x 9 doubles, in the caller's order.  The host form takes
 * HOST pointers and returns when the outputs are written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_flow(fmmbem_plan *plan, int p, const double *x /* n x 3 */,
                             double *u /* n_targets x 3 or NULL */, double *q /* n_targets or NULL */,
                             double *G /* n_targets x 9 or NULL */);
int fmmbem_plan_execute_flow_device(fmmbem_plan *plan, int p, const double *d_x,
                                    double *d_u, double *d_q, double *d_G, void *stream);

/* ---- Representation execute: both Laplace layers at the points of a target plan, value and gradient, in one pass --------------
 * (no reference counterpart).  The representation formula of a Laplace BEM solution off the surface is
 * phi(t) = (S[sigma](t) - D[mu](t)) / 4 pi, S the single layer of the density sigma and D the double layer of the surface
 * potential mu; its gradient is the physical field.  On a Laplace plan over separate targets (fmmbem_plan_create_targets,
 * fmmbem_plan_create_field), for target i at the point t_i:
 *   phi_i  = sum_j E0(t_i, s_j) sigma_j - sum_j E1(t_i, s_j) mu_j
 *   grad_i = sum_j gamma0(t_i, s_j) sigma_j - sum_j gamma1(t_i, s_j) mu_j          (three doubles: d/dt_x, d/dt_y, d/dt_z)
 * E0 / E1: the entries fmmbem_kernel_entries gives for a flag-0 / flag-1 target in every regime (the K stored points; semi-analytic
 * G and the 16-point rule on the vertices; the 2 pi self value of dG/dn); gamma0 / gamma1: those of fmmbem_plan_execute_gradient.
 * Put differently: phi is fmmbem_plan_execute(sigma) on the all-flag-0 plan over the points minus fmmbem_plan_execute(mu) on the
 * all-flag-1 plan, grad the same with fmmbem_plan_execute_gradient -- to rounding (1e-12 relative to the two layers' norms), not
 * bit for bit: the near sums are accumulated in another association and the far field is one expansion instead of two.  The
 * scaling is execute's: the physical values are the results / 4 pi.
 * THE TARGETS' OWN FLAGS DO NOT ENTER: every target gets both layers at its point; copies of a point that differ only in flag
 * receive identical bits.  A null density or potential leaves that layer out; a null output is not computed.
 * One call is: one gather per layer, P2M per layer given into that layer's slot of M, the two slots FOLDED into one multipole set
 * at the leaves (M0 += M1), ONE far chain through L2L on slot 0 alone -- the cost of one potential execute's far field for both
 * layers, value and gradient --, ONE kernel over the near pairs (a panel's record staged once, one regime test per pair, one
 * y_q - t, |d_q|^2 and reciprocal square root per quadrature point feeding all four integrands, a row's four sums in list order),
 * the value's and the gradient's L2P kernels on L0, the delivery.  Its buffers are allocated at first use: mu in tree order, the
 * value's tree / points / staging buffers, the gradient's (those of fmmbem_plan_execute_gradient), and the P2M moment table of a
 * slot the plan's own targets do not make live -- FMMBEM_ERR_ALLOC if that fails, the plan stays usable; where the plan's own
 * P2M runs without a table, so does this one.  Launched plainly, kernel by kernel, whatever fmmbem_plan_set_graphs says; the
 * captured graphs of execute are left as they are, and execute, execute_batch and execute_gradient return the same bits before
 * and after it.  The same bits on every run.
 * Checked in this order: a null plan -> FMMBEM_ERR_INVALID; density and potential both null, or phi and grad both null ->
 * _INVALID; p outside 1..p_max -> _INVALID; a plan that is not over separate targets -> _UNSUPPORTED; a Stokes plan ->
 * _UNSUPPORTED; a host-only plan -> _UNSUPPORTED; a treecode plan (it has no local expansions) -> _UNSUPPORTED.  A refusal touches
 * no pointer and leaves the handle usable.
 * With stage timing on it is recorded as ONE execute: ms_p2m covers the P2M launches and the fold, ms_near the near kernel,
 * ms_l2p the L2P kernels, the other stages as in a field execute.  No batches, no graphs, no shards, no device lists.
 * density, potential: n_panels doubles; phi: n_targets, grad: n_targets x 3 doubles, in the caller's order.  The host form takes
 * HOST pointers and returns when the outputs are written; the device form is asynchronous on `stream`. */
int fmmbem_plan_execute_representation(fmmbem_plan *plan, int p,
                                       const double *density /* n_panels or NULL */, const double *potential /* n_panels or NULL */,
                                       double *phi /* n_targets or NULL */, double *grad /* n_targets x 3 or NULL */);
int fmmbem_plan_execute_representation_device(fmmbem_plan *plan, int p, const double *d_density, const double *d_potential,
                                              double *d_phi, double *d_grad, void *stream);

/* ---- exact block-Jacobi preconditioner: z = M v with M = the inverse of the block-diagonal operator ----------------------
 * (no reference counterpart: Preconditioners::BlockDiagonal, examples/BEM/BlockDiagonalPC.hpp:16-60, runs ONE inner GMRES
 * iteration on that operator instead).  A BLOCK_DIAGONAL plan holds every leaf's self block assembled in HBM; build inverts
 * each of them once on the device -- Gauss-Jordan with partial pivoting, the pivot the largest magnitude of its column, the
 * lowest row among equals -- into storage of its own; apply is then one streaming pass over the inverses (8 bytes per entry of
 * the blocks) for up to 4 vectors at a time.  fmmbem_plan_execute on the plan is unchanged: it applies the blocks.
 *   build: the plan must have been created with evaluator FMMBEM_EVAL_BLOCK_DIAGONAL and sparse_local = 1 on one device with
 *     shard_world = 1.  Checked in this order: null -> FMMBEM_ERR_INVALID; another evaluator or a target plan -> _INVALID;
 *     matrix-free, a device list or a shard -> _UNSUPPORTED; host-only -> _NO_DEVICE; a leaf of more than
 *     FMMBEM_BLOCK_INVERSE_MAX unknowns (ncrit * dof) -> _UNSUPPORTED.  A zero or non-finite pivot -> _INVALID, the message names
 *     the leaf, and the plan stays usable with no inverse attached.  A second build on a plan that has its inverse returns OK.
 *   apply: vector j is v + j*ldv, result j is z + j*ldz, n_panels x dof doubles each in the caller's panel order; v and z must
 *     not overlap; every entry of z is written.  Row r of a leaf's result is acc = fma(M(r, c), v_c, acc) over the leaf's
 *     columns c in ascending order from acc = 0: the bits depend on the inputs only, not on k or on the run.  k < 1, a null
 *     pointer, a leading dimension shorter than a vector, or a plan without an inverse: FMMBEM_ERR_INVALID.  The device form is
 *     asynchronous on `stream`; the host form returns when z is written.
 *   bytes: HBM bytes of the inverses (0 before build); fmmbem_stats reports none of them. */
#define FMMBEM_BLOCK_INVERSE_MAX 768
int fmmbem_plan_block_inverse_build(fmmbem_plan *block_diagonal_plan);
int fmmbem_plan_block_inverse_apply_device(fmmbem_plan *plan, int k, const double *d_v, size_t ldv,
                                           double *d_z, size_t ldz, void *stream);
int fmmbem_plan_block_inverse_apply(fmmbem_plan *plan, int k, const double *v, size_t ldv, double *z, size_t ldz);
int fmmbem_plan_block_inverse_bytes(const fmmbem_plan *plan, int64_t *bytes);

/* Toggle per-stage HIP-event timing.  While enabled every execute records HIP events around each
 * kernel on the stream it runs on (no synchronisation is added); fmmbem_plan_stats() waits for the
 * recorded events and reports the mean stage times of up to the last 64 executes.  Enabling resets
 * the record.  Default off. */
int fmmbem_plan_set_timing(fmmbem_plan *plan, int enabled);      /* 0 off; 1 every stage; 2 the near-field kernel only */

/* Replay the launch chain of an execute (everything between the gather of x and the delivery of y) as a hipGraph per order p,
 * captured the second time the plan runs at that order and launched on the caller's stream from then on: one host call
 * instead of ~16.  Same kernels, same order, same bits.  Off by default (also FMMBEM_GRAPH=1 at creation); executes with
 * stage timing on are not graphed.  Environment switches that the launchers read per launch are frozen into a captured
 * graph. */
int fmmbem_plan_set_graphs(fmmbem_plan *plan, int enabled);

int fmmbem_plan_stats(const fmmbem_plan *plan, fmmbem_stats *out);

/* ---- introspection (tests, partition checks) --------------------------------------------- */
/* Body::number() permutation, tree index -> original index (Octree.hpp:298-300). out: n_panels. */
int fmmbem_plan_get_perm(const fmmbem_plan *plan, uint32_t *out);
/* Boxes in BFS order. Any pointer may be NULL. center: n_boxes x 3. */
int fmmbem_plan_get_boxes(const fmmbem_plan *plan, double *center, double *side, int32_t *level,
                          int32_t *is_leaf, int32_t *parent, int32_t *body_begin, int32_t *body_end);
/* Pair lists; which: 0 = P2P (source leaf, target leaf), 1 = M2L (source box, target box),
 * 2 = M2M (child, parent), 3 = L2L (parent, child); the work list of the rotation M2L kernel: 4 = its OWNED pairs (source
 * box, target box) in the order the kernel takes them, 5 = its items as (first, one past last) positions in list 4 (the
 * short cut, orders with several wavefronts per SIMD), 6 = the long cut of the same list (orders p >= 9).
 * out may be NULL; returns the count via *n. */
int fmmbem_plan_get_pairs(const fmmbem_plan *plan, int which, int32_t *out, int64_t *n);
/* One assembled near-matrix row (tree-order index of the unknown, i.e. dof*panel + component; must be
 * owned): column indices (same numbering) and values, ascending columns.  cols/vals may be NULL; *n
 * receives the row length. */
int fmmbem_plan_get_near_row(const fmmbem_plan *plan, int64_t row, uint32_t *cols, double *vals,
                             int64_t *n);
/* Diagonal of the assembled near matrix = the self-interactions K(s,s) that Preconditioners::Diagonal inverts
 * (examples/BEM/Preconditioner.hpp:19-42; examples/LaplaceBEM.cpp:241-244): out[n_panels * dof], original order;
 * rows of other shards are returned as zero. */
int fmmbem_plan_get_diagonal(const fmmbem_plan *plan, double *out);

/* Kernel::operator()(target, source) for n independent panel pairs (kernel/LaplaceSphericalBEM.hpp:273-297,
 * kernel/StokesSphericalBEM.hpp:377-389): the panel integral of source i seen from the centroid of target i, evaluated on
 * the device by the code that assembles the near matrix.  Reads opts->kernel, quad_k, quad_k_fine, mu, device.
 * target_vertices / source_vertices: n x 9; target_bc: n flags or NULL (the TARGET's flag selects G vs dG/dn, :282-291);
 * out: n doubles (Laplace) or n row-major 3x3 blocks (Stokes).  No plan is needed: this is what Preconditioners::Diagonal
 * (examples/BEM/Preconditioner.hpp:24-33) calls as K(*it, *it) on the panels of FMM_plan::source_begin(). */
int fmmbem_kernel_entries(const fmmbem_options *opts, size_t n, const double *target_vertices, const uint8_t *target_bc,
                          const double *source_vertices, double *out);
/* gamma(target, source) of the field gradient (see fmmbem_plan_execute_gradient) for n independent pairs, by the function the
 * gradient execute's near kernel calls: the target POINT is the centroid of target_vertices' panel i, target_bc its flag (NULL:
 * all 0).  Laplace only (FMMBEM_ERR_UNSUPPORTED otherwise); reads opts->kernel, quad_k, device.  out: n x 3. */
int fmmbem_kernel_gradient_entries(const fmmbem_options *opts, size_t n, const double *target_vertices,
                                   const uint8_t *target_bc, const double *source_vertices, double *out /* n x 3 */);
/* eta(target, source) of the field Hessian (see fmmbem_plan_execute_hessian) for n independent pairs, by the function the Hessian
 * execute's near kernel calls: the target POINT is the centroid of target_vertices' panel i, target_bc its flag (NULL: all 0).
 * Laplace only (FMMBEM_ERR_UNSUPPORTED otherwise); reads opts->kernel, quad_k, device.  out: n x 9, [a][b], symmetric bit for bit. */
int fmmbem_kernel_hessian_entries(const fmmbem_options *opts, size_t n, const double *target_vertices,
                                  const uint8_t *target_bc, const double *source_vertices, double *out /* n x 9 */);
/* pi(target, source) of the field pressure (see fmmbem_plan_execute_pressure) for n independent pairs, by the function the
 * pressure execute's near kernel calls: the target POINT is the centroid of target_vertices' panel i.  Stokes only
 * (FMMBEM_ERR_UNSUPPORTED otherwise); reads opts->kernel, quad_k, quad_k_fine, device.  out: n x 3. */
int fmmbem_kernel_pressure_entries(const fmmbem_options *opts, size_t n, const double *target_vertices,
                                   const double *source_vertices, double *out /* n x 3 */);
/* Gamma(target, source) of the field velocity gradient (see fmmbem_plan_execute_velocity_gradient) for n independent pairs, by
 * the function the execute's near kernel calls, with f left open: G[k][m] += sum_e out[k][m][e] f_e, the 1/(2 mu) included.  The
 * target POINT is the centroid of target_vertices' panel i.  Stokes only (FMMBEM_ERR_UNSUPPORTED otherwise); reads opts->kernel,
 * mu, quad_k, quad_k_fine, device.  out: n x 27, [k][m][e]. */
int fmmbem_kernel_velocity_gradient_entries(const fmmbem_options *opts, size_t n, const double *target_vertices,
                                            const double *source_vertices, double *out /* n x 27 */);

/* ---- the translation operators one at a time: the KernelSkeleton contract (kernel/KernelSkeleton.hpp:62-212) --------------
 * What the reference's kernel classes offer beside operator(): P2M, M2M, M2L, L2L, L2P as kernel/LaplaceSphericalBEM.hpp:307-476
 * and kernel/StokesSphericalBEM.hpp:391-530 define them (each "+=" into its last argument), for code that drives single operators
 * (tests/single_level.cpp, ExpansionTraits<K>::is_valid_fmm of include/KernelTraits.hpp:188-194).  Every call runs the SAME device
 * kernels a plan's matvec runs, on a two-box plan that holds just the call's operands (csrc/ops.hip); operands and results are
 * host buffers.  M2P (the treecode's operator) runs inside a plan created with FMMBEM_EVAL_TREECODE and is
 * not offered as a single operator.
 *   fmmbem_ops_create reads opts->kernel, p_max (1..16), quad_k, mu, device.  A handle is not thread-safe.
 *   An expansion: [slot][p (p + 1) / 2] complex as (re, im) pairs, coefficient (n, m >= 0) at n (n + 1) / 2 + m -- the reference's
 *   stored half (kernel/LaplaceSpherical.hpp:187-206).  fmmbem_ops_slots: the slots P2M writes and L2P reads -- Laplace 2
 *   (multipole_type[0] = G moments of POTENTIAL sources, [1] = dG/dn moments of NORMAL_DERIV sources, :323-344; L2P adds r0 at a
 *   POTENTIAL target and subtracts r1 at a NORMAL_DERIV target, :448-476), Stokes 4 (the stokeslet group M[0][0..3] of VELOCITY
 *   sources, StokesSphericalBEM.hpp:414-430; L2P at VELOCITY targets with the 1 / (2 mu), :512-522).  Stokes TRACTION sources
 *   and targets are FMMBEM_ERR_UNSUPPORTED here: the reference's stresslet moments (:432-466) are not the far field this library
 *   computes for those rows (see FMMBEM_KERNEL_STOKES_BEM above).
 *   M2M / M2L / L2L act on n_slots (1..12) expansions alike -- pass both groups of a Stokes multipole_type as 8.
 *   translation = centre of the target expansion - centre of the source expansion (executor/M2M.hpp, M2L.hpp:40, L2L.hpp).
 *   vertices: n x 9; bc: n flags or NULL (all 0); charges: n x dof; result: n x dof, added to. */
typedef struct fmmbem_ops fmmbem_ops;
int fmmbem_ops_create(const fmmbem_options *opts, fmmbem_ops **out);
void fmmbem_ops_destroy(fmmbem_ops *ops);
int fmmbem_ops_slots(const fmmbem_ops *ops);
int fmmbem_ops_p2m(fmmbem_ops *ops, int p, size_t n, const double *vertices, const uint8_t *bc, const double *charges,
                   const double center[3], double *M);
int fmmbem_ops_m2m(fmmbem_ops *ops, int p, int n_slots, const double *M_source, double *M_target, const double translation[3]);
int fmmbem_ops_m2l(fmmbem_ops *ops, int p, int n_slots, const double *M_source, double *L_target, const double translation[3]);
int fmmbem_ops_l2l(fmmbem_ops *ops, int p, int n_slots, const double *L_source, double *L_target, const double translation[3]);
int fmmbem_ops_l2p(fmmbem_ops *ops, int p, const double *L, const double center[3], size_t n, const double *vertices,
                   const uint8_t *bc, double *result);

/* ---- Direct sum: y_i = sum_j K(t_i, s_j) x_j over ALL sources, on the device (Direct::matvec, include/Direct.hpp:232-302) ----
 * The O(N M) sum the reference checks its FMM and its exterior field against, with every entry the one fmmbem_kernel_entries gives
 * for that pair, summed where it is made (csrc/kernels_direct.hip).  No tree, no matrix: the handle holds the source panels in the
 * caller's order.  Laplace and Stokes; for Stokes this is the route to velocity / double-layer values at points off the surface.
 *   fmmbem_direct_create reads opts->kernel, quad_k, quad_k_fine, mu, device.  source_vertices: n_sources x 9.
 *   target_points: n_targets x 3, or NULL for the symmetric form (Direct.hpp:291-302): the targets are the sources' own centroids as
 *     the device computed them, n_targets must equal n_sources and target_bc holds the panels' flags.
 *   target_bc: n_targets flags or NULL (all 0).  The TARGET's flag picks the operator -- Laplace G or dG/dn; Stokes velocity, or the
 *     double layer with the SOURCE's normal -- the sources carry no flags.
 *   x: n_sources x dof, y: n_targets x dof (dof = 3 for Stokes), y is OVERWRITTEN.
 * Order of addition, fixed: the sources are cut into chunks of fmmbem_direct_chunk() consecutive panels; a target's partial sum over
 * a chunk is acc = fma(K_ij, x_j, acc) in ascending j from 0 (Stokes: per component, the block's columns 0, 1, 2 of source j in
 * turn); y_i is the partial sums added in ascending chunk order.  A result's bits therefore depend on the inputs only -- not on
 * n_targets, on how a set of targets is split over calls, or on the run.
 * Errors: null arguments, n == 0, a bad quadrature key, mu <= 0 (Stokes), a vertex or target point that is not finite, n_targets !=
 * n_sources in the symmetric form: FMMBEM_ERR_INVALID from one host pass before any device is touched (the _device form cannot read
 * its points and checks the rest); no device: FMMBEM_ERR_NO_DEVICE.  The partial sums live in a buffer the handle owns and grows on
 * demand (at most 256 MB: more targets are served in slabs); if growing fails the call returns FMMBEM_ERR_ALLOC, the buffer is
 * left empty and the handle stays usable.  fmmbem_direct_apply_device is asynchronous on `stream`; a handle is not thread-safe. */
typedef struct fmmbem_direct fmmbem_direct;
int fmmbem_direct_create(const fmmbem_options *opts, size_t n_sources, const double *source_vertices, fmmbem_direct **out);
int fmmbem_direct_apply(fmmbem_direct *direct, size_t n_targets, const double *target_points, const uint8_t *target_bc,
                        const double *x, double *y);
int fmmbem_direct_apply_device(fmmbem_direct *direct, size_t n_targets, const double *d_target_points, const uint8_t *d_target_bc,
                               const double *d_x, double *d_y, void *stream);
int fmmbem_direct_chunk(void);
void fmmbem_direct_destroy(fmmbem_direct *direct);

/* ---- Direct sum: field quantities -- the gradient, the pressure and the velocity gradient at points, over ALL sources ---------
 * The exact sums the field executes above approximate: on a handle of fmmbem_direct_create, for target point t_i (target_points:
 * n_targets x 3, required: there is no symmetric form),
 *   fmmbem_direct_gradient            Laplace handles only.  g_i = sum_j gamma(t_i, s_j) x_j, three doubles per target; gamma is that
 *                                     of fmmbem_plan_execute_gradient, picked by target_bc[i] (NULL: all 0).
 *   fmmbem_direct_pressure            Stokes handles only, no flags.  q_i = sum_j pi(t_i, s_j) . x_j, one double per target; pi and
 *                                     the scaling are those of fmmbem_plan_execute_pressure.
 *   fmmbem_direct_velocity_gradient   Stokes handles only, no flags.  G_i[k][m], nine doubles per target, row-major; the tensor and
 *                                     the scaling (the 1/(2 mu) included) are those of fmmbem_plan_execute_velocity_gradient.
 * Every pair's value is the one the field executes' near kernels and fmmbem_kernel_{gradient,pressure,velocity_gradient}_entries
 * compute, in every regime (self, the fine rule on the vertices, the K stored points).  x: n_sources x dof, as for apply; the
 * outputs are OVERWRITTEN.  The host forms take HOST pointers and return when the result is written; the _device forms take
 * device pointers and are asynchronous on `stream`.
 * Order of addition, fixed: the chunks of fmmbem_direct_chunk() consecutive sources, ascending j within a chunk from zero sums, the
 * chunks' partial sums added in ascending chunk order, as for apply.  Within a chunk
 *   gradient            acc_c = fma(gamma_c, x_j, acc_c), c = 0, 1, 2;
 *   pressure            acc = fma(pi_x, x_j0, acc), then pi_y x_j1, then pi_z x_j2;
 *   velocity gradient   every pair is added straight into the chunk's nine sums, each quadrature point's tensor contracted with
 *                       f = x_j in place and unscaled, points in order; the nine sums are multiplied by 1/2/mu once, where the
 *                       chunk's partial sum is stored.  With one source and x = e_e these are the operations of
 *                       fmmbem_kernel_velocity_gradient_entries: the result is its column e, bit for bit.
 * A result's bits therefore depend on the inputs only -- not on n_targets, on how a set of targets is split over calls, or on the
 * run.
 * Checked in this order: a null handle, points, x or output -> FMMBEM_ERR_INVALID; n_targets == 0 -> _INVALID; the wrong kind of
 * handle (gradient on a Stokes handle; pressure or velocity gradient on a Laplace handle) -> FMMBEM_ERR_UNSUPPORTED, the message
 * naming the quantity and the kernel it needs; host forms only: a target point that is not finite -> _INVALID.  On every refusal
 * the output is untouched and the handle stays usable.  The partial sums live in the handle's buffer, as for apply (width 3, 1 or
 * 9 doubles per chunk and target; at most 256 MB, more targets are served in slabs); if growing it fails: FMMBEM_ERR_ALLOC, the
 * buffer is left empty and the handle stays usable. */
int fmmbem_direct_gradient(fmmbem_direct *direct, size_t n_targets, const double *target_points, const uint8_t *target_bc,
                           const double *x, double *g /* n_targets x 3 */);
int fmmbem_direct_gradient_device(fmmbem_direct *direct, size_t n_targets, const double *d_target_points, const uint8_t *d_target_bc,
                                  const double *d_x, double *d_g, void *stream);
/* The Hessian of the Laplace field over ALL sources: H_i[a][b] = sum_j eta_ab(t_i, s_j) x_j, nine doubles per target, row-major; eta
 * is that of fmmbem_plan_execute_hessian, picked by target_bc[i] (NULL: all 0), every pair's value the one
 * fmmbem_kernel_hessian_entries gives.  Laplace handles only.  The gradient's chunks and order: within a chunk
 * acc_c = fma(eta_c, x_j, acc_c) for the six components of the upper triangle in ascending j from zero sums, the chunks' partial sums
 * added in ascending chunk order, mirrored where they are stored: H[a][b] and H[b][a] carry the same bits, and with one source and
 * x = 1 the result is the entry bit for bit.  The checks, their order and the buffer are those of fmmbem_direct_gradient (a Stokes
 * handle -> FMMBEM_ERR_UNSUPPORTED naming the Hessian; 9 doubles per chunk and target). */
int fmmbem_direct_hessian(fmmbem_direct *direct, size_t n_targets, const double *target_points, const uint8_t *target_bc,
                          const double *x, double *H /* n_targets x 9 */);
int fmmbem_direct_hessian_device(fmmbem_direct *direct, size_t n_targets, const double *d_target_points, const uint8_t *d_target_bc,
                                 const double *d_x, double *d_H, void *stream);
int fmmbem_direct_pressure(fmmbem_direct *direct, size_t n_targets, const double *target_points, const double *x /* n x 3 */,
                           double *q /* n_targets */);
int fmmbem_direct_pressure_device(fmmbem_direct *direct, size_t n_targets, const double *d_target_points, const double *d_x,
                                  double *d_q, void *stream);
int fmmbem_direct_velocity_gradient(fmmbem_direct *direct, size_t n_targets, const double *target_points, const double *x /* n x 3 */,
                                    double *G /* n_targets x 9 */);
int fmmbem_direct_velocity_gradient_device(fmmbem_direct *direct, size_t n_targets, const double *d_target_points, const double *d_x,
                                           double *d_G, void *stream);

/* ---- the orthogonalisation step of the callers above the matvec (examples/BEM/GMRES.hpp:203-212: modified Gram-Schmidt of
 * w against V_0 .. V_{ncols-1}, then the normalised next basis vector), device vectors, ONE call per Arnoldi column:
 *   for k < ncols:  h[k] = <w, V_k>;  w -= h[k] V_k;      h[ncols] = |w|;   vnext = w / h[ncols]
 * d_V: ncols vectors of n doubles, ldv apart; d_h: ncols + 1 doubles on the device; d_scratch:
 * fmmbem_mgs_scratch_doubles(largest ncols) doubles of work space (no initial contents assumed; reusable across calls and
 * sizes); asynchronous on `stream`.  The sums are formed in a fixed order.  Vectors that start on 16-byte boundaries with an
 * even ldv take the vector path; anything else is correct but scalar. */
int fmmbem_mgs_column_device(int64_t n, double *d_w, const double *d_V, int64_t ldv, int ncols, double *d_h, double *d_vnext,
                             double *d_scratch, void *stream);
int fmmbem_mgs_scratch_doubles(int max_cols);

/* ---- the caller of the hot path, resident on the device: restarted GMRES / flexible GMRES with the per-iteration relaxation
 * of the expansion order p (examples/BEM/GMRES.hpp:143-252 GMRES, :276-380 FGMRES; examples/BEM/GMRES_Stokes.hpp:173-320 the
 * same loops on Vec<3,double> values with the Stokes order rule; examples/BEM/SolverOptions.hpp:11-39).  The Krylov basis V
 * (and Z of FGMRES) lives in HBM, every matvec is fmmbem_plan_execute_device, every Arnoldi column one
 * fmmbem_mgs_column_device; the Hessenberg column comes to the host once per iteration (its only synchronisation) for the
 * Givens rotations, the residual estimate and predict_p; restart, back substitution and the solution update as the reference.
 * The same steps in the same order as the reference's loop -- order schedule, iteration counts and printed residuals are
 * the reference's (tests/golden/gmres_ref_r*.json) -- only the association inside a dot product differs. */
typedef enum { FMMBEM_RELAX_SIMONCINI = 0, FMMBEM_RELAX_BOURAS = 1 } fmmbem_relaxation;   /* SolverOptions::relaxation_type */
typedef enum {
  FMMBEM_ORDER_GMRES = 0,          /* GMRES.hpp:195         p = max(1, predict_p(|r|))                                    */
  FMMBEM_ORDER_GMRES_STOKES = 1,   /* GMRES_Stokes.hpp:229  p = max(p_min, predict_p(|r|) - 1)                            */
  FMMBEM_ORDER_FGMRES = 2,         /* GMRES.hpp:324         p = predict_p(|r|)  (raised to 1: the library has no order 0)   */
  FMMBEM_ORDER_FGMRES_STOKES = 3   /* GMRES_Stokes.hpp:373  p = max(5, predict_p(|r|))                                     */
} fmmbem_order_rule;

typedef struct {
  double  residual;        /* SolverOptions::residual: stop when |r| / |b| falls below it                               */
  int32_t max_iters;       /* SolverOptions::max_iters                                                                 */
  int32_t restart;         /* SolverOptions::restart (the drivers set it to max_iters, LaplaceBEM.cpp:162-163)          */
  int32_t max_p, p_min;    /* SolverOptions::max_p, p_min                                                              */
  int32_t variable_p;      /* SolverOptions::variable_p: 0 = every matvec at max_p                                     */
  int32_t relax_type;      /* fmmbem_relaxation                                                                        */
  int32_t order_rule;      /* fmmbem_order_rule: which call site's floor is applied to predict_p                       */
  int32_t flexible;        /* 0 GMRES (x += y_j M(V_j), the preconditioner applied again in the update, GMRES.hpp:237-241);
                            * 1 FGMRES (Z_j = M(V_j) kept, x += y_j Z_j, :318-320, :368-371)                           */
  int32_t initial_p;       /* the order of the FIRST matvec r0 = A x0 - b, run before any predict_p: the reference uses whatever
                            * the kernel object holds (its construction order); 0 = max_p                               */
} fmmbem_solver_options;
void fmmbem_solver_options_default(fmmbem_solver_options *opts);   /* SolverOptions(): 1e-5, 500, 500, 16, 5, true, BOURAS */

typedef enum {
  FMMBEM_PC_IDENTITY = 0,    /* Preconditioners::Identity (Preconditioner.hpp:8-17)                                       */
  FMMBEM_PC_DIAGONAL = 1,    /* Preconditioners::Diagonal (:19-42): z = reciprocals .* v, in whatever order the caller built them */
  FMMBEM_PC_INNER_PLAN = 2,  /* Preconditioners::LocalInnerSolver / BlockDiagonal (LocalPC.hpp:26-59, BlockDiagonalPC.hpp:16-60):
                              * z = GMRES(inner_plan, 0, v, inner) on a plan created with evaluator LOCAL or BLOCK_DIAGONAL */
  FMMBEM_PC_BLOCK_INVERSE = 3 /* z = fmmbem_plan_block_inverse_apply_device(inner_plan, v): inner_plan = a BLOCK_DIAGONAL plan of the
                              * same panels on the same device with its inverse built; .inner is ignored.  M is exact, constant and
                              * linear: plain GMRES applies it once per column and ONCE to the combination sum_c y_c V_c in the
                              * solution update */
} fmmbem_preconditioner_kind;
typedef struct {
  int32_t kind;                      /* fmmbem_preconditioner_kind                                                     */
  const double *reciprocals;         /* DIAGONAL: n_panels * dof values; a DEVICE pointer for fmmbem_gmres_device, a host
                                      * pointer for fmmbem_gmres                                                       */
  fmmbem_plan *inner_plan;           /* INNER_PLAN, BLOCK_INVERSE: same panels, same device                            */
  fmmbem_solver_options inner;       /* INNER_PLAN: LocalPC.hpp:52-54 uses residual 1e-1, variable_p 0, max_iters 1     */
} fmmbem_preconditioner;

typedef struct {
  int32_t iterations;                /* out: matvecs of the inner loops (the reference's `iter`)                        */
  double  residual;                  /* out: last |r| / |b| estimate                                                  */
  double  seconds;                   /* out: wall time of the call, the final synchronisation included                 */
  int32_t capacity;                  /* in: entries p[] / resid[] can take (0 or NULL arrays: no history)              */
  int32_t *p;                        /* out: order of iteration k (what the reference prints as fmm_req_p)             */
  double  *resid;                    /* out: |r| / |b| after iteration k                                               */
} fmmbem_solver_log;

/* x: initial guess in, solution out; b: right-hand side; n_panels * dof doubles each, ORIGINAL panel order, DEVICE pointers.
 * M == NULL: identity.  log may be NULL.  Synchronises `stream` once per iteration and before returning. */
int fmmbem_gmres_device(fmmbem_plan *plan, const fmmbem_solver_options *opts, double *d_x, const double *d_b,
                        const fmmbem_preconditioner *M, fmmbem_solver_log *log, void *stream);
/* The same with HOST pointers (x, b, M->reciprocals): the vectors cross PCIe once each way per solve, not per matvec. */
int fmmbem_gmres(fmmbem_plan *plan, const fmmbem_solver_options *opts, double *x, const double *b,
                 const fmmbem_preconditioner *M, fmmbem_solver_log *log);

/* Several right-hand sides on one plan: k INDEPENDENT solves of the loop above, advanced in lockstep -- not a block Krylov
 * method: every system keeps its own Krylov space, Hessenberg matrix, rotations, residual estimate and relaxed order.  For
 * every system j the solution, iterations, residual and the p[] / resid[] histories are bit for bit what
 * fmmbem_gmres_device(plan, opts, x_j, b_j, M, &logs[j]) gives for it alone.  What the k systems share is the work per
 * iteration: the matvecs of the systems that ask for the same order go through one fmmbem_plan_execute_batch_device (one pass
 * over the near-field matrix where fmmbem_plan_batch_width > 1), the Arnoldi columns of all of them are one chain of i + 3
 * launches (per 64 systems) and reach the host in one copy behind one synchronisation.  Restart length and max_iters are
 * common; a system that converges leaves, the others restart together.
 * System j is x + j*ldx (initial guess in, solution out) and b + j*ldb, n_panels * dof doubles each, ORIGINAL panel order; the
 * doubles between vectors are neither read nor written.  logs: NULL or k logs, each used as fmmbem_gmres uses its one (seconds:
 * the wall time of the whole call).  One set of options and one preconditioner serve all systems; an INNER_PLAN
 * preconditioner's inner solves are themselves one batched solve on the inner plan.
 * k < 1, a null pointer, ldx or ldb shorter than a vector: FMMBEM_ERR_INVALID, checked first; everything else is refused as
 * fmmbem_gmres(_device) refuses it.  fmmbem_gmres(_device) is this solver with k = 1.  The plan keeps one workspace for all
 * its solves, as wide as the widest so far (k times that of one system); if growing it fails the call returns
 * FMMBEM_ERR_ALLOC, the workspace is left empty and the next solve, of any k, allocates again. */
int fmmbem_gmres_batch_device(fmmbem_plan *plan, const fmmbem_solver_options *opts, int k,
                              double *d_x, size_t ldx, const double *d_b, size_t ldb,
                              const fmmbem_preconditioner *M, fmmbem_solver_log *logs, void *stream);
int fmmbem_gmres_batch(fmmbem_plan *plan, const fmmbem_solver_options *opts, int k,
                       double *x, size_t ldx, const double *b, size_t ldb,
                       const fmmbem_preconditioner *M, fmmbem_solver_log *logs);

/* ---- split execute of a plan created with shard_upward = 1 and shard_world > 1 (no reference counterpart:
 * the reference is single-node) ----------------------------------------------------------
 *   upward:   x -> P2M and M2M of the boxes this shard owns -> d_send (exchange_doubles(p) doubles)
 *   caller:   all-gather of the shards' d_send into d_recv (shard_world x exchange_doubles(p), rank order)
 *             [meanwhile, optionally: near_split -> y]
 *   downward: d_recv -> the remaining M2M, M2L, L2L, L2P and the near field -> y (zero outside the owned rows) */
int fmmbem_plan_exchange_doubles(const fmmbem_plan *plan, int p, size_t *per_shard);
/* shard_upward = 2: the same split execute, but the caller's collective is ONE all-to-all with uneven counts that carries,
 * for every pair of shards, only the multipoles the receiver's lists read (the M2L sources of its targets and the private
 * children of the few parents every shard translates): 2-3 thousand boxes per shard instead of 60 thousand at N = 1M on 8
 * shards.  send_doubles[q] / recv_doubles[q], q < shard_world: doubles this shard sends to / receives from shard q at order p
 * (0 for itself); d_send / d_recv of upward / downward hold the peers' segments one after the other, rank order -- the
 * layout of MPI_Alltoallv / torch.distributed.all_to_all_single with split sizes. */
int fmmbem_plan_exchange_counts(const fmmbem_plan *plan, int p, int64_t *send_doubles, int64_t *recv_doubles);
int fmmbem_plan_upward_device(fmmbem_plan *plan, int p, const double *d_x, double *d_send, void *stream);
int fmmbem_plan_downward_device(fmmbem_plan *plan, int p, const double *d_recv, double *d_y, void *stream);
/* Optional, between the two: the near field of this shard (y = A_near x of the x given to upward; zero outside the owned
 * rows), so that it runs while the caller's all-gather is in flight.  downward then skips it and adds the far field. */
int fmmbem_plan_near_split_device(fmmbem_plan *plan, double *d_y, void *stream);

/* The result as a slice instead of a zero-padded vector (the shards' rows are disjoint and, in tree
 * order, contiguous -- an all-gather moves half the bytes of the all-reduce).  With result slices enabled, every execute /
 * downward call writes only the rows this shard owns, in TREE order, to d_y[0 .. rows * dof); the caller all-gathers the
 * shards' slices into chunks of `chunk_doubles` (rank order; chunk >= the largest slice) and
 * fmmbem_plan_assemble_slices_device puts them into ORIGINAL panel order: y[n_panels * dof].  The values are the ones the
 * zero-padded form holds, bit for bit.  fmmbem_plan_shard_rows: cut[shard_world + 1], shard r owns tree rows
 * [cut[r], cut[r+1]) (every rank builds the same tree, so every rank knows all cuts). */
int fmmbem_plan_set_result_slices(fmmbem_plan *plan, int enabled);
int fmmbem_plan_shard_rows(const fmmbem_plan *plan, int64_t *cut);
int fmmbem_plan_assemble_slices_device(fmmbem_plan *plan, const double *d_slices, size_t chunk_doubles, double *d_y, void *stream);

/* Multipole (which=0) or local (which=1) coefficients of the last execute for every box:
 * out[box][slot][p(p+1)/2][re,im]; slots = fmmbem_stats.expansion_slots: Laplace 2 (G, dG/dn); Stokes 8 (M[2][4]), or 11 when
 * the plan has TRACTION targets (slots 4..10: the seven dipole potentials of the double layer). */
int fmmbem_plan_get_expansions(const fmmbem_plan *plan, int which, int p, double *out);

/* ---- mesh generator of the reference's drivers ------------------------------------------- */
/* Triangulation::UnitSphere(panels, recursions) (examples/BEM/Triangulation.hpp:105-121):
 * N = 2*4^recursions panels.  vertices == NULL: only returns N through *n_panels. */
int fmmbem_mesh_unit_sphere(int recursions, double *vertices, size_t *n_panels);
/* Triangulation::RedBloodCell(panels, recursions) with identity rotation and zero shift
 * (examples/BEM/Triangulation.hpp:184-255; examples/StokesBEM.cpp:111-113): same N, same calling convention. */
int fmmbem_mesh_red_blood_cell(int recursions, double *vertices, size_t *n_panels);
/* Triangulation::MultipleRedBloodCell(panels, recursions, cells) (examples/BEM/Triangulation.hpp:260-321): N =
 * cells * 2*4^recursions.  placement: cells x {alpha, beta, gamma, shift x, y, z} (RotationMatrix, :142-163), or NULL for
 * the reference's own drand48-driven orientations and offsets (see csrc/mesh_io.cpp for what that sequence assumes). */
int fmmbem_mesh_red_blood_cells(int recursions, int cells, const double *placement, double *vertices, size_t *n_panels);

/* Triangle Gauss rule `key` of examples/BEM/GaussQuadrature.hpp:15-274 (what BEMConfig hands the kernels): barycentric
 * points[n][3] and weights[n], n <= FMMBEM_MAX_QUAD (size the buffers for that); either array may be NULL.
 * Keys: 1 3 4 7 (alias of 4, :58-59) 13 17 (16 points) 19 25 79. */
#define FMMBEM_MAX_QUAD 79
int fmmbem_quadrature(int key, double *points, double *weights, int *n);

/* ---- mesh files of the reference's drivers ------------------------------------------------ */
/* All readers: vertices == NULL only counts (*n_panels out); otherwise *n_panels holds the capacity of
 * vertices (panels) on entry and the number read on return; vertices[panel][vertex][xyz].
 * MeshIO::readMsh (examples/BEM/MshReader.hpp:18-94): gmsh format 2 ASCII; elements of type 2 (triangles) only,
 * stored in element-number order with the winding swapped (v1, v3, v2) as the reference does. */
int fmmbem_mesh_read_msh(const char *path, double *vertices, size_t *n_panels);
/* MeshIO::ReadVertFace (examples/BEM/VertFaceReader.hpp:17-76): count line then "x y z" lines; count line then
 * 1-indexed "v1 v2 v3" lines; winding kept. */
int fmmbem_mesh_read_vert_face(const char *vert_path, const char *face_path, double *vertices, size_t *n_panels);
/* The .vert/.face pair the generators dump (examples/BEM/Triangulation.hpp:124-134), three vertices per
 * triangle, written WITH the count lines ReadVertFace expects and 17 significant digits. */
int fmmbem_mesh_write_vert_face(const char *vert_path, const char *face_path, const double *vertices, size_t n_panels);

/* ---- errors ------------------------------------------------------------------------------ */
const char *fmmbem_status_string(int status);
const char *fmmbem_last_error(void);
int fmmbem_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FMMBEM_H */
