/* fmm_oracle.h -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * A plain-C restatement of the reference's LaplaceSphericalBEM FMM matvec path
 * (barbagroup/fmm-bem-relaxed).  Every function cites the reference file:line it
 * follows.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may load this library; the product (fmm-bem-relaxed_amd/) never does.
 *
 * PARITY STATUS: the reference's FMM cannot be built in this image (it needs
 * Boost, which is absent, and stand-in headers are not allowed), and its
 * repository holds no golden vectors.  Per-element parity of the MATVEC is
 * therefore UNPINNED.  What IS pinned: the reference-run known answers recorded
 * in SURVEY.md section 6 (exact list statistics for r=6,8,9; FMM-vs-Direct error
 * levels at p=5,8,10,12), checked by tests/test_oracle_known_answers.py;
 * analytic identities per operator (tests/test_analytic_operators.py); and, for
 * the CALLER of the path, the reference's own GMRES.hpp compiled unmodified
 * around this oracle's matvec (ref_gmres_driver.cpp -> _ref/ref_gmres,
 * fixtures tests/golden/gmres_ref_r*.json).
 *
 * TARGET PLANS (targets.c): the reference declares FMM_plan(K, sources, targets, opts) and never builds it, so nothing of the
 * reference can pin them.  targets.c is a second derivation of the product's documented contract from this oracle's own
 * pieces (orc_tree_build twice over one root cube, orc_dual_walk between the trees, every source in every live slot, the
 * complete L2L rule, L2P at the point, orc_eval_G / orc_eval_dGdn by the target's flag); its lists are checked against the
 * product's entry for entry (tests/test_target_plan_oracle_host.py) and its matvec against the GPU row by row
 * (tests/test_gpu_target_plan_oracle.py).  With targets at the centroids and one flag it IS the single oracle with the
 * complete L2L rule (to 1e-13, tested).
 */
#ifndef FMM_ORACLE_H
#define FMM_ORACLE_H

#include <complex.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#error "the oracle is plain C"
#endif

#define ORC_MAXK 80      /* max stored quadrature points per panel            */
#define ORC_PMAX 20      /* max expansion order the stack buffers allow       */
#define ORC_EPS 1e-12    /* kernel/LaplaceSpherical.hpp:30                     */

typedef double complex cplx;

enum { ORC_POTENTIAL = 0, ORC_NORMAL_DERIV = 1 };

/* kernel/LaplaceSphericalBEM.hpp:38-118 (Panel), flattened */
typedef struct {
  double v[3][3];          /* vertices                                         */
  double c[3];             /* centroid                                         */
  double n[3];             /* unit normal                                      */
  double area;
  const double (*q)[3];    /* stored quadrature points (nq of them; storage owned by the ctx) */
  int bc;                  /* ORC_POTENTIAL / ORC_NORMAL_DERIV                 */
} orc_panel;

/* include/tree/Octree.hpp:201-269 (box_data), plus derived geometry */
typedef struct {
  uint64_t key;            /* marker-bit Morton key, leaf bit stripped         */
  uint32_t parent;
  uint32_t cb, ce;         /* children (box ids) or bodies (tree ids) if leaf  */
  int leaf;
  int level;
  double center[3];
  double side;             /* side_length()                                    */
  uint32_t bb, be;         /* body range in tree order (all boxes)             */
} orc_box;

typedef struct { int first, second; } orc_pair;

/* one octree on its own (tree.c orc_tree_build): the single plan's tree, or either tree of a target plan */
typedef struct {
  int n;                   /* bodies                                           */
  double pmin[3], cell[3];
  unsigned levels;         /* bits per dimension of the coder: 10 or 21        */
  int nboxes, nlevels;
  orc_box *boxes;          /* BFS order                                        */
  uint32_t *perm;          /* tree index -> body index                         */
  uint64_t *code;
  int *level_offset;       /* nlevels+1 entries                                */
} orc_tree;

typedef struct orc_ctx {
  /* inputs */
  int n;                   /* panels                                           */
  int K;                   /* quadrature key as the user gave it               */
  int nq;                  /* actual number of stored quadrature points        */
  double qw[ORC_MAXK];     /* weights of the K rule                            */
  double theta;
  unsigned ncrit;
  orc_panel *panels;       /* ORIGINAL order                                   */
  double *quad;            /* n * nq * 3 quadrature point storage              */
  /* tree */
  double pmin[3], cell[3];
  int nboxes, nlevels;     /* nlevels = Octree::levels()                       */
  orc_box *boxes;
  uint32_t *perm;          /* tree index -> original index (Body::number())    */
  uint64_t *code;          /* Morton code per tree index                       */
  unsigned levels;         /* bits per dimension of the coder: 10 (reference) or 21 (tree.c DEEP_LEVELS) */
  int *level_offset;       /* nlevels+1 entries                                */
  /* lists: executor/EvalInteractionLazySparse.hpp:37-47 */
  orc_pair *p2p; int n_p2p;        /* (source leaf, target leaf)               */
  orc_pair *lr;  int n_lr;         /* (source box, target box)                 */
  int *p2m; int n_p2m;
  orc_pair *m2m; int n_m2m;        /* (child, parent) in reference order       */
  orc_pair *l2l; int n_l2l;        /* (parent, child) in reference order       */
  int *l2p; int n_l2p;
  int n_l2l_skipped;       /* parent->child edges the reference's lazy rule omits
                              although the parent holds a local expansion      */
  /* LR list regrouped by target (canonical, race-free order) */
  int *lr_ptr, *lr_src;    /* nboxes+1, n_lr                                   */
  /* near matrix, CSR, rows/cols in tree order: executor/EvalP2P.hpp:47-98    */
  int64_t *row_ptr; uint32_t *col; double *val; int64_t nnz;
  /* expansions (allocated for pcap) */
  int pcap;
  cplx *M, *L;             /* [box][2][pcap*(pcap+1)/2]                        */
  /* Stokes (stokes.c): viscosity, near-regime rule K_fine, 3x3 near blocks, 2x4 expansions */
  double mu; int kfine, nqf; double qfp[ORC_MAXK][3], qfw[ORC_MAXK];
  double *val9; int spcap; cplx *MS, *LS;
} orc_ctx;

/* precomputed tables of LaplaceSpherical (kernel/LaplaceSpherical.hpp:87-117) */
typedef struct {
  int P;
  double *prefactor;       /* 4P^2 */
  double *Anm;             /* 4P^2 */
  cplx *Cnm;               /* P^4  */
} orc_tables;

/* ---- geometry.c ---- */
int  orc_quadrature(int key, double pts[][3], double *w);   /* returns #points, -1 bad key */
void orc_panel_init(orc_panel *p, const double v[9], int bc, int nq, const double pts[][3], double *qstore);
long orc_unit_sphere(int recursions, double *verts_out);    /* verts_out may be NULL: returns N */
double orc_eval_G(const orc_panel *s, const double t[3], int nq, const double *w);
double orc_eval_dGdn(const orc_panel *s, const double t[3], int nq, const double *w);
double orc_kernel(const orc_ctx *c, const orc_panel *t, const orc_panel *s);
void orc_semi_analytical(double *G, double *dGdn, const double y0[3], const double y1[3],
                         const double y2[3], const double x[3], int same);

/* ---- tree.c ---- */
int  orc_tree_build(orc_tree *t, int n, const double *pts, const double pmin[3], const double mx[3], unsigned levels,
                    unsigned ncrit);
void orc_tree_free(orc_tree *t);
void orc_dual_walk(const orc_tree *S, const orc_tree *T, double theta, int keep_lr, orc_pair **p2p, int *n_p2p,
                   orc_pair **lr, int *n_lr);
enum { ORC_EVAL_FMM = 0, ORC_EVAL_LOCAL = 1, ORC_EVAL_BLOCK_DIAGONAL = 2 };
orc_ctx *orc_create_eval(int n, const double *verts, const uint8_t *bc, int K, double theta, unsigned ncrit, int evaluator);
orc_ctx *orc_create(int n, const double *verts, const uint8_t *bc, int K, double theta,
                    unsigned ncrit);
void orc_complete_l2l(orc_ctx *c);   /* not a reference rule: see tree.c */
void orc_destroy(orc_ctx *c);
void orc_stats(const orc_ctx *c, int64_t out[16]);

/* ---- expansions.c ---- */
orc_tables *orc_tables_create(int P);
void orc_tables_destroy(orc_tables *t);
void orc_cart2sph(double *r, double *theta, double *phi, const double d[3]);
void orc_eval_multipole(const orc_tables *t, double rho, double alpha, double beta,
                        cplx *Ynm, cplx *YnmTheta);
void orc_eval_local(const orc_tables *t, double rho, double alpha, double beta,
                    cplx *Ynm, cplx *YnmTheta);
void orc_p2m_panel(const orc_tables *t, const orc_panel *src, int nq, const double *qw,
                   double charge, const double center[3], cplx *M0, cplx *M1);
void orc_m2m(const orc_tables *t, const cplx *Ms, cplx *Mt, const double tr[3]);
void orc_m2l(const orc_tables *t, const cplx *Ms, cplx *Lt, const double tr[3]);
void orc_l2l(const orc_tables *t, const cplx *Ls, cplx *Lt, const double tr[3]);
void orc_l2p_panel(const orc_tables *t, const cplx *L0, const cplx *L1, const double center[3],
                   const orc_panel *tgt, double *result);

/* ---- matvec.c ---- */
int  orc_build_near(orc_ctx *c);
int  orc_build_near_pattern(orc_ctx *c);    /* row_ptr/col only */
int  orc_matvec(orc_ctx *c, int P, const double *x, double *y, int flags, double stage_s[8]);
void orc_direct(const orc_ctx *c, const double *x, double *y, int row_begin, int row_end);
void orc_direct_rows(const orc_ctx *c, const double *x, double *y_out, int nrows, const int32_t *rows);
void orc_near_only(const orc_ctx *c, const double *x, double *y);

/* ---- stokes.c ---- */
int  orc_stokes_config(orc_ctx *c, double mu, int kfine);
void orc_stokes_entry(const orc_ctx *c, const orc_panel *t, const orc_panel *s, double out[9]);
int  orc_stokes_build_near(orc_ctx *c);
int  orc_stokes_matvec(orc_ctx *c, int P, const double *x, double *y, int flags, double stage_s[8]);
void orc_stokes_direct(const orc_ctx *c, const double *x, double *y, int row_begin, int row_end);
void orc_stokes_direct_rows(const orc_ctx *c, const double *x, double *y_out, int nrows, const int32_t *rows);
void orc_red_blood_cell_map(long n, double *verts);
/* single P2M / L2P on caller-supplied panels (kernel 0 Laplace [2][S], 1 Stokes velocity group [4][S]); += */
int orc_single_p2m(int kernel, int P, int K, double mu, int n, const double *verts, const uint8_t *bc, const double *charges,
                   const double center[3], cplx *M);
int orc_single_l2p(int kernel, int P, int K, double mu, const cplx *L, const double center[3], int n, const double *verts,
                   const uint8_t *bc, double *result);

/* ---- targets.c: an FMM over separate target points (NOT a reference path: the reference declares FMM_plan(K, sources,
 * targets, opts), include/FMM_plan.hpp:45-55, and never builds it).  y_i = sum_j K(t_i, s_j) x_j, the target's flag picking
 * G or dG/dn.  Two trees on one root cube, the dual walk of tree.c between them, every source in every live expansion slot,
 * the complete L2L rule on the target tree. ---- */
typedef struct orc_tctx {
  int n;                   /* source panels                                    */
  int nt;                  /* targets as given                                 */
  int np;                  /* distinct targets (point, flag), first-occurrence order */
  int K, nq;
  double qw[ORC_MAXK];
  double theta;
  unsigned ncrit;
  orc_panel *panels;       /* ORIGINAL order; bc unused                        */
  double *quad;
  double *pts;             /* np x 3                                           */
  uint8_t *flag;           /* np                                               */
  uint32_t *point_of;      /* nt: given target -> distinct target              */
  double pmin[3];
  orc_tree S, T;           /* source tree (panel centroids), target tree (distinct points) */
  orc_pair *p2p; int n_p2p;        /* (S leaf, T leaf), walk order             */
  orc_pair *lr;  int n_lr;         /* (S box, T box), walk order               */
  orc_pair *m2m; int n_m2m;        /* (S child, S parent), post-order          */
  orc_pair *l2l; int n_l2l;        /* (T parent, T child), BFS order           */
  int *p2m; int n_p2m;             /* S leaves that need a multipole           */
  char *hasL;                      /* per T box                                */
  int live[2];                     /* slot 0 (G) / 1 (dG/dn) read by some target */
  int *lr_ptr, *lr_src;            /* M2L grouped by T box                     */
  int *near_ptr, *near_src;        /* per T box: its P2P source leaves, ascending body range */
} orc_tctx;

orc_tctx *orc_target_create(int n, const double *verts, int nt, const double *pts, const uint8_t *flags, int K, double theta,
                            unsigned ncrit);
void orc_target_destroy(orc_tctx *c);
int  orc_target_matvec(const orc_tctx *c, int P, const double *x, double *y);
void orc_target_direct(const orc_tctx *c, const double *x, double *y);

#define ORC_FLAG_FAITHFUL 1   /* both expansions, serial SpMV/M2M/L2L like the reference */
#define ORC_FLAG_TARGET_RANGE 2

#endif
