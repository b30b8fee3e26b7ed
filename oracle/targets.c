/* targets.c -- CPU ORACLE (test infrastructure): the FMM over separate target points, built from the oracle's own pieces --
 * tree.c's octree and dual walk, expansions.c's operators, geometry.c's entries.  NOT a reference path (the reference
 * declares FMM_plan(K, sources, targets, opts), include/FMM_plan.hpp:45-55, and never builds it); the contract it restates:
 *
 *   - distinct targets: identical coordinates with the same flag are one body, represented by their first occurrence;
 *     distinct targets are numbered in first-occurrence order, results come back in the given order, duplicates copied;
 *   - one root cube over the panel centroids and the distinct targets (the single plan's rule, Octree.hpp:67-79), one ncrit,
 *     one coder: 10 bits for both trees unless either needs more, then 21 for both;
 *   - the dual walk of tree.c from the pair of roots, source tree against target tree;
 *   - P2M of every source into every live slot (0: G, 1: dG/dn; live = some target carries that flag); M2M on the source
 *     tree, M2L source box -> target box, L2L every parent -> child edge of the target tree below a box that holds L, L2P at
 *     the point about its leaf's centre in the slot of its flag; near pairs K(t, s) = orc_eval_G / orc_eval_dGdn by the
 *     target's flag.
 * See fmm_oracle.h for the rules. */
#include "fmm_oracle.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define LEVELS 10u
#define DEEP_LEVELS 21u

/* distinct targets: sort given indices by (x, y, z, flag, index); equal neighbours are one body */
static const double *g_pts;
static const uint8_t *g_flags;
static int tflag(int k) { return g_flags && g_flags[k] ? 1 : 0; }
static int cmp_target(const void *a, const void *b) {
  const int i = *(const int *)a, j = *(const int *)b;
  for (int k = 0; k < 3; ++k) {
    const double x = g_pts[3*(size_t)i + k], y = g_pts[3*(size_t)j + k];
    if (x < y) return -1;
    if (x > y) return 1;
  }
  if (tflag(i) != tflag(j)) return tflag(i) - tflag(j);
  return (i > j) - (i < j);
}
static int same_target(int i, int j) {
  return g_pts[3*(size_t)i] == g_pts[3*(size_t)j] && g_pts[3*(size_t)i + 1] == g_pts[3*(size_t)j + 1] &&
         g_pts[3*(size_t)i + 2] == g_pts[3*(size_t)j + 2] && tflag(i) == tflag(j);
}

/* EvalInteractionLazySparse.hpp:173-194 (resolve_multipole) on the source tree */
static void need_multipole(const orc_tree *S, int b, char *initM, int **p2m, int *n_p2m, orc_pair **m2m, int *n_m2m) {
  if (initM[b]) return;
  const orc_box *bx = &S->boxes[b];
  if (bx->leaf) {
    (*p2m)[(*n_p2m)++] = b;
  } else {
    for (uint32_t ch = bx->cb; ch < bx->ce; ++ch) {
      need_multipole(S, (int)ch, initM, p2m, n_p2m, m2m, n_m2m);
      (*m2m)[(*n_m2m)++] = (orc_pair){ (int)ch, b };
    }
  }
  initM[b] = 1;
}

/* a CSR of pairs by their second (target) box; firsts kept in list order */
static void group_by_target(const orc_pair *p, int np, int nboxes, int **ptr_out, int **src_out) {
  int *ptr = calloc((size_t)nboxes + 1, sizeof(int));
  int *src = malloc(sizeof(int)*(size_t)(np ? np : 1));
  for (int i = 0; i < np; ++i) ptr[p[i].second + 1]++;
  for (int b = 0; b < nboxes; ++b) ptr[b+1] += ptr[b];
  int *fill = malloc(sizeof(int)*(size_t)nboxes);
  memcpy(fill, ptr, sizeof(int)*(size_t)nboxes);
  for (int i = 0; i < np; ++i) src[fill[p[i].second]++] = p[i].first;
  free(fill);
  *ptr_out = ptr; *src_out = src;
}

orc_tctx *orc_target_create(int n, const double *verts, int nt, const double *pts, const uint8_t *flags, int K, double theta,
                            unsigned ncrit) {
  double qp[ORC_MAXK][3];
  if (n <= 0 || nt <= 0) return NULL;
  for (size_t k = 0; k < 3*(size_t)nt; ++k) if (!isfinite(pts[k])) return NULL;
  orc_tctx *c = calloc(1, sizeof(*c));
  c->n = n; c->nt = nt; c->K = K; c->theta = theta; c->ncrit = ncrit;
  c->nq = orc_quadrature(K, qp, c->qw);
  if (c->nq < 0) { free(c); return NULL; }
  c->panels = malloc(sizeof(orc_panel)*(size_t)n);
  c->quad = malloc(sizeof(double)*3*(size_t)c->nq*(size_t)n);
  for (int i = 0; i < n; ++i)
    orc_panel_init(&c->panels[i], verts + 9*(size_t)i, 0, c->nq, qp, c->quad + 3*(size_t)c->nq*(size_t)i);

  /* ---- distinct targets ---- */
  int *order = malloc(sizeof(int)*(size_t)nt), *rep = malloc(sizeof(int)*(size_t)nt);
  for (int k = 0; k < nt; ++k) order[k] = k;
  g_pts = pts; g_flags = flags;
  qsort(order, (size_t)nt, sizeof(int), cmp_target);
  for (int i = 0; i < nt;) {
    int j = i + 1;
    while (j < nt && same_target(order[i], order[j])) ++j;
    for (int k = i; k < j; ++k) rep[order[k]] = order[i];      /* sorted by index within a group: order[i] comes first */
    i = j;
  }
  c->point_of = malloc(sizeof(uint32_t)*(size_t)nt);
  c->pts = malloc(sizeof(double)*3*(size_t)nt);
  c->flag = malloc((size_t)nt);
  c->np = 0;
  for (int k = 0; k < nt; ++k) {
    if (rep[k] == k) {
      c->point_of[k] = (uint32_t)c->np;
      memcpy(c->pts + 3*(size_t)c->np, pts + 3*(size_t)k, sizeof(double)*3);
      c->flag[c->np] = (uint8_t)tflag(k);
      c->np++;
    } else {
      c->point_of[k] = c->point_of[rep[k]];
    }
  }
  free(order); free(rep);
  g_pts = NULL; g_flags = NULL;
  for (int i = 0; i < c->np; ++i) c->live[c->flag[i]] = 1;

  /* ---- one root cube over the centroids and the distinct targets ---- */
  double *cen = malloc(sizeof(double)*3*(size_t)n);
  double mn[3], mx[3];
  for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) cen[3*i + k] = c->panels[i].c[k];
  for (int k = 0; k < 3; ++k) mn[k] = mx[k] = cen[k];
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) { mn[k] = fmin(mn[k], cen[3*i + k]); mx[k] = fmax(mx[k], cen[3*i + k]); }
  for (int i = 0; i < c->np; ++i)
    for (int k = 0; k < 3; ++k) { mn[k] = fmin(mn[k], c->pts[3*i + k]); mx[k] = fmax(mx[k], c->pts[3*i + k]); }
  double ext = fmax(fabs(mx[0]-mn[0]), fmax(fabs(mx[1]-mn[1]), fabs(mx[2]-mn[2])));
  for (int k = 0; k < 3; ++k) {
    mx[k] = fmax(mx[k], mn[k] + ext*(1 + 1e-6));
    c->pmin[k] = mn[k];
  }

  /* ---- two trees, one coder ---- */
  if (orc_tree_build(&c->S, n, cen, c->pmin, mx, LEVELS, ncrit) || orc_tree_build(&c->T, c->np, c->pts, c->pmin, mx, LEVELS, ncrit)) {
    orc_tree_free(&c->S); orc_tree_free(&c->T);
    orc_tree_build(&c->S, n, cen, c->pmin, mx, DEEP_LEVELS, ncrit);
    orc_tree_build(&c->T, c->np, c->pts, c->pmin, mx, DEEP_LEVELS, ncrit);
  }
  free(cen);

  /* ---- the walk, source tree against target tree ---- */
  orc_dual_walk(&c->S, &c->T, theta, 1, &c->p2p, &c->n_p2p, &c->lr, &c->n_lr);

  /* ---- multipoles wanted: M2L sources and their subtrees ---- */
  char *initM = calloc((size_t)c->S.nboxes, 1);
  c->p2m = malloc(sizeof(int)*(size_t)c->S.nboxes);
  c->m2m = malloc(sizeof(orc_pair)*(size_t)c->S.nboxes);
  for (int i = 0; i < c->n_lr; ++i) need_multipole(&c->S, c->lr[i].first, initM, &c->p2m, &c->n_p2m, &c->m2m, &c->n_m2m);
  free(initM);

  /* ---- locals: every M2L target, and everything below it (the complete L2L rule, tree.c orc_complete_l2l) ---- */
  c->hasL = calloc((size_t)c->T.nboxes, 1);
  for (int i = 0; i < c->n_lr; ++i) c->hasL[c->lr[i].second] = 1;
  c->l2l = malloc(sizeof(orc_pair)*(size_t)c->T.nboxes);
  for (int b = 1; b < c->T.nboxes; ++b)
    if (c->hasL[c->T.boxes[b].parent]) {
      c->hasL[b] = 1;
      c->l2l[c->n_l2l++] = (orc_pair){ (int)c->T.boxes[b].parent, b };
    }

  group_by_target(c->lr, c->n_lr, c->T.nboxes, &c->lr_ptr, &c->lr_src);
  group_by_target(c->p2p, c->n_p2p, c->T.nboxes, &c->near_ptr, &c->near_src);
  for (int b = 0; b < c->T.nboxes; ++b) {            /* near columns ascending (EvalP2P.hpp:87) */
    int *s = c->near_src + c->near_ptr[b]; const int m = c->near_ptr[b+1] - c->near_ptr[b];
    for (int i = 1; i < m; ++i) {
      int v = s[i], j = i - 1;
      while (j >= 0 && c->S.boxes[s[j]].bb > c->S.boxes[v].bb) { s[j+1] = s[j]; --j; }
      s[j+1] = v;
    }
  }
  return c;
}

void orc_target_destroy(orc_tctx *c) {
  if (!c) return;
  free(c->panels); free(c->quad); free(c->pts); free(c->flag); free(c->point_of);
  orc_tree_free(&c->S); orc_tree_free(&c->T);
  free(c->p2p); free(c->lr); free(c->m2m); free(c->l2l); free(c->p2m); free(c->hasL);
  free(c->lr_ptr); free(c->lr_src); free(c->near_ptr); free(c->near_src);
  free(c);
}

static double target_entry(const orc_tctx *c, int point, const orc_panel *s) {
  const double *t = c->pts + 3*(size_t)point;
  return c->flag[point] == ORC_POTENTIAL ? orc_eval_G(s, t, c->nq, c->qw) : orc_eval_dGdn(s, t, c->nq, c->qw);
}

/* y (given order, nt values) = the FMM at order P.  y is OVERWRITTEN. */
int orc_target_matvec(const orc_tctx *c, int P, const double *x, double *y) {
  if (P < 1 || P > ORC_PMAX) return -1;
  const int S = P*(P+1)/2, nbs = c->S.nboxes, nbt = c->T.nboxes;
  orc_tables *t = orc_tables_create(P);
  cplx *M = calloc((size_t)nbs*2*S, sizeof(cplx)), *L = calloc((size_t)nbt*2*S, sizeof(cplx));
  double *yp = calloc((size_t)c->np, sizeof(double));
  if (!t || !M || !L || !yp) { orc_tables_destroy(t); free(M); free(L); free(yp); return -2; }
  /* near field: per target leaf, its source leaves in ascending body order */
  #pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < nbt; ++b) {
    const orc_box *tb = &c->T.boxes[b];
    if (!tb->leaf) continue;
    for (uint32_t i = tb->bb; i < tb->be; ++i) {
      const int pt = (int)c->T.perm[i];
      double r = 0;
      for (int k = c->near_ptr[b]; k < c->near_ptr[b+1]; ++k) {
        const orc_box *sb = &c->S.boxes[c->near_src[k]];
        for (uint32_t j = sb->bb; j < sb->be; ++j) r += target_entry(c, pt, &c->panels[c->S.perm[j]]) * x[c->S.perm[j]];
      }
      yp[pt] = r;
    }
  }
  /* P2M: every source into every live slot */
  #pragma omp parallel for schedule(dynamic, 4)
  for (int i = 0; i < c->n_p2m; ++i) {
    const orc_box *b = &c->S.boxes[c->p2m[i]];
    cplx *M0 = M + ((size_t)c->p2m[i]*2 + 0)*S, *M1 = M0 + S;
    for (uint32_t j = b->bb; j < b->be; ++j)
      for (int e = 0; e < 2; ++e) {
        if (!c->live[e]) continue;
        orc_panel src = c->panels[c->S.perm[j]];
        src.bc = e;
        orc_p2m_panel(t, &src, c->nq, c->qw, x[c->S.perm[j]], b->center, M0, M1);
      }
  }
  /* M2M, post-order */
  for (int i = 0; i < c->n_m2m; ++i) {
    const int ch = c->m2m[i].first, pa = c->m2m[i].second;
    double tr[3]; for (int k = 0; k < 3; ++k) tr[k] = c->S.boxes[pa].center[k] - c->S.boxes[ch].center[k];
    for (int e = 0; e < 2; ++e)
      if (c->live[e]) orc_m2m(t, M + ((size_t)ch*2 + e)*S, M + ((size_t)pa*2 + e)*S, tr);
  }
  /* M2L, by target box, sources in walk order */
  #pragma omp parallel for schedule(dynamic, 8)
  for (int b = 0; b < nbt; ++b) {
    for (int i = c->lr_ptr[b]; i < c->lr_ptr[b+1]; ++i) {
      const int s = c->lr_src[i];
      double tr[3]; for (int k = 0; k < 3; ++k) tr[k] = c->T.boxes[b].center[k] - c->S.boxes[s].center[k];
      for (int e = 0; e < 2; ++e)
        if (c->live[e]) orc_m2l(t, M + ((size_t)s*2 + e)*S, L + ((size_t)b*2 + e)*S, tr);
    }
  }
  /* L2L, parents first */
  for (int i = 0; i < c->n_l2l; ++i) {
    const int pa = c->l2l[i].first, ch = c->l2l[i].second;
    double tr[3]; for (int k = 0; k < 3; ++k) tr[k] = c->T.boxes[ch].center[k] - c->T.boxes[pa].center[k];
    for (int e = 0; e < 2; ++e)
      if (c->live[e]) orc_l2l(t, L + ((size_t)pa*2 + e)*S, L + ((size_t)ch*2 + e)*S, tr);
  }
  /* L2P at the point, about its leaf's centre, in the slot of its flag */
  #pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < nbt; ++b) {
    const orc_box *tb = &c->T.boxes[b];
    if (!tb->leaf || !c->hasL[b]) continue;
    const cplx *L0 = L + ((size_t)b*2 + 0)*S, *L1 = L0 + S;
    for (uint32_t i = tb->bb; i < tb->be; ++i) {
      const int pt = (int)c->T.perm[i];
      orc_panel tgt; memset(&tgt, 0, sizeof tgt);
      memcpy(tgt.c, c->pts + 3*(size_t)pt, sizeof(double)*3);
      tgt.bc = c->flag[pt];
      orc_l2p_panel(t, L0, L1, tb->center, &tgt, &yp[pt]);
    }
  }
  for (int k = 0; k < c->nt; ++k) y[k] = yp[c->point_of[k]];
  free(M); free(L); free(yp);
  orc_tables_destroy(t);
  return 0;
}

/* y (given order) = sum_j K(t_i, s_j) x_j over every panel, at the exact points (include/Direct.hpp:99-125's sum) */
void orc_target_direct(const orc_tctx *c, const double *x, double *y) {
  double *yp = malloc(sizeof(double)*(size_t)c->np);
  #pragma omp parallel for schedule(dynamic, 4)
  for (int i = 0; i < c->np; ++i) {
    double r = 0;
    for (int j = 0; j < c->n; ++j) r += target_entry(c, i, &c->panels[j]) * x[j];
    yp[i] = r;
  }
  for (int k = 0; k < c->nt; ++k) y[k] = yp[c->point_of[k]];
  free(yp);
}

/* ---- accessors for the ctypes wrapper ---- */
/* n_panels, n_targets, n_target_points, n_source_boxes, n_source_leaves, n_source_levels, n_target_boxes, n_target_leaves,
 * n_target_levels, tree_coder_levels, p2p, m2l, m2m, l2l, p2m leaves, live slots (bit 0: G, bit 1: dG/dn) */
void orc_target_info(const orc_tctx *c, int64_t out[16]) {
  int ls = 0, lt = 0;
  for (int b = 0; b < c->S.nboxes; ++b) ls += c->S.boxes[b].leaf;
  for (int b = 0; b < c->T.nboxes; ++b) lt += c->T.boxes[b].leaf;
  out[0] = c->n; out[1] = c->nt; out[2] = c->np;
  out[3] = c->S.nboxes; out[4] = ls; out[5] = c->S.nlevels;
  out[6] = c->T.nboxes; out[7] = lt; out[8] = c->T.nlevels;
  out[9] = c->S.levels;
  out[10] = c->n_p2p; out[11] = c->n_lr; out[12] = c->n_m2m; out[13] = c->n_l2l; out[14] = c->n_p2m;
  out[15] = c->live[0] | (c->live[1] << 1);
}

/* tree 0: source, 1: target; bodies counted from 0 in that tree; a root is its own parent (0) */
void orc_target_boxes(const orc_tctx *c, int tree, double *center, double *side, int32_t *level, int32_t *leaf, int32_t *parent,
                      int32_t *bb, int32_t *be) {
  const orc_tree *T = tree ? &c->T : &c->S;
  for (int b = 0; b < T->nboxes; ++b) {
    const orc_box *x = &T->boxes[b];
    memcpy(center + 3*b, x->center, sizeof(double)*3);
    side[b] = x->side; level[b] = x->level; leaf[b] = x->leaf; parent[b] = (int32_t)x->parent;
    bb[b] = (int32_t)x->bb; be[b] = (int32_t)x->be;
  }
}

/* which: 0 p2p (S leaf, T leaf), 1 m2l (S box, T box), 2 m2m (S child, S parent), 3 l2l (T parent, T child) */
int orc_target_pairs(const orc_tctx *c, int which, int32_t *out) {
  const orc_pair *p; int n;
  switch (which) {
    case 0: p = c->p2p; n = c->n_p2p; break;
    case 1: p = c->lr;  n = c->n_lr;  break;
    case 2: p = c->m2m; n = c->n_m2m; break;
    case 3: p = c->l2l; n = c->n_l2l; break;
    default: return -1;
  }
  if (out) for (int i = 0; i < n; ++i) { out[2*i] = p[i].first; out[2*i+1] = p[i].second; }
  return n;
}

/* source tree -> panel, target tree -> distinct target, given target -> distinct target; the distinct targets' points and flags */
void orc_target_perm(const orc_tctx *c, uint32_t *src_perm, uint32_t *tgt_perm, uint32_t *point_of, double *pts, uint8_t *flags) {
  if (src_perm) memcpy(src_perm, c->S.perm, sizeof(uint32_t)*(size_t)c->n);
  if (tgt_perm) memcpy(tgt_perm, c->T.perm, sizeof(uint32_t)*(size_t)c->np);
  if (point_of) memcpy(point_of, c->point_of, sizeof(uint32_t)*(size_t)c->nt);
  if (pts) memcpy(pts, c->pts, sizeof(double)*3*(size_t)c->np);
  if (flags) memcpy(flags, c->flag, (size_t)c->np);
}
