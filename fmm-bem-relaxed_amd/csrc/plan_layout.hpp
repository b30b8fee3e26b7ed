// plan_layout.hpp -- what a plan's device arrays hold, decided on the host: every list, record and class table that
// to_device_near / to_device_far (plan.hip) upload, as a pure function of the host plan and a few plain options.  No HIP call, no
// switch, no environment: plan.hip fills LayoutOptions in one place, calls near_layout / far_layout and uploads the fields in
// order.  Host code only (plain g++ compiles it; tests/test_plan_layout_host.py runs it without a device).
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "device_plan.hpp"
#include "host_plan.hpp"
#include "host_tables.hpp"
#include "launch_choice.hpp"
#include "shift_lanes.hpp"

namespace fmmbem {

// What the layouts take from the caller's options, the run-time switches and the kernels' translation units
struct LayoutOptions {
  int dof = 1;                          // unknowns per panel: 1 Laplace, 3 Stokes
  bool sparse_local = true;             // the near field is a stored matrix (false: matrix-free)
  bool treecode = false;                // FMMBEM_EVAL_TREECODE
  bool targets = false;                 // a dual plan (HostPlan::build_targets)
  double near_stream_fraction = 1.0;    // the option, or FMMBEM_NEAR_STREAM_FRACTION
  bool stokes_sym = true;               // FMMBEM_STOKES_SYM
  bool m2l_rot = true;                  // FMMBEM_M2L_ROT
  int near_f32_max_p = 0;
  int rcg_item_rows = 60;               // rows an item of near_recompute3g_kernel may hold (kernels_near.hip)
  int l2p_group_leaves = 8;             // most leaves of an L2P work group (kernels_far.hip)
};

// the class tables of a plan are a few thousand independent rows of harmonics: a few threads take them in contiguous shares
template <class F>
inline void parallel_rows(int64_t n, int64_t min_per_thread, F&& body) {
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency())), n / std::max<int64_t>(1, min_per_thread)));
  if (nt <= 1) { body((int64_t)0, n); return; }
  host_parallel(nt, [&](int t) { body(n * t / nt, n * (t + 1) / nt); });
}

// Work items largest first, equal ones in their given order: a stable radix sort on the (descending) key -- the comparison
// sort of 60 000 items took 4-5 ms of every plan build
template <class T, class KeyFn>
inline void stable_sort_largest_first(std::vector<T>& v, KeyFn key) {
  if (v.size() < 2) return;
  uint64_t kmax = 0;
  for (const T& x : v) kmax = std::max<uint64_t>(kmax, (uint64_t)key(x));
  std::vector<T> tmp(v.size());
  constexpr int kBits = 11, kB = 1 << kBits;
  for (int shift = 0; shift < 64 && (kmax >> shift) != 0; shift += kBits) {
    size_t count[kB + 1] = {0};
    for (const T& x : v) ++count[(((kmax - (uint64_t)key(x)) >> shift) & (kB - 1)) + 1];
    for (int b = 0; b < kB; ++b) count[b + 1] += count[b];
    for (const T& x : v) tmp[count[((kmax - (uint64_t)key(x)) >> shift) & (kB - 1)]++] = x;
    v.swap(tmp);
  }
}

// ---------------------------------------- the cutters ----------------------------------------
struct WorkItem { int leaf, r0, nr; int64_t key; };   // rows [r0, r0 + nr) of a leaf; key: what the items are sorted by (bytes, pairs)

// Rows of one leaf's block cut into ranges of <= item_bytes, so that no workgroup is left streaming one coarse leaf alone: as many
// whole rows as fit, a multiple of 8 (fewer than 8 fit: ranges of min(4, rows), processed with the columns split over the
// wavefronts instead of the rows), then dealt evenly over that many ranges, again rounded up to 8.  Appends (leaf, r0, nr, bytes).
inline void cut_rows(int leaf, int rows, int64_t row_bytes, int64_t item_bytes, std::vector<WorkItem>& out) {
  int per = (int)std::max<int64_t>(1, item_bytes / row_bytes);
  if (per >= 8) per &= ~7; else per = std::min(4, rows);
  const int cnt = (rows + per - 1) / per;
  per = (rows + cnt - 1) / cnt;
  if (per >= 8) per = (per + 7) & ~7;
  for (int r0 = 0; r0 < rows; r0 += per) { const int k = std::min(per, rows - r0); out.push_back({leaf, r0, k, k * row_bytes}); }
}
// Rows of a recomputed leaf in ranges of <= cap rows, dealt evenly (the kernel gives a wavefront ceil(rows / 4) of an item's rows).
// Appends (leaf, r0, nr, pairs).
inline void cut_recompute(int leaf, int rows, int ncp, int cap, std::vector<WorkItem>& out) {
  const int cnt = (rows + cap - 1) / cap;
  const int per = (rows + cnt - 1) / cnt;
  for (int r0 = 0; r0 < rows; r0 += per) { const int k = std::min(per, rows - r0); out.push_back({leaf, r0, k, (int64_t)k * ncp}); }
}
// Work items of near_side_items (kernels_near.hip): runs of consecutive rows that hold <= 256 listed entries together (a workgroup
// takes the entries one per thread, then a thread per row adds the row's products in entry order), at most 256 rows; a row of
// more than 256 is an item of its own, taken 256 at a time; an empty row ends a run.  (first entry, one past the last, first row,
// one past the last)
inline std::vector<int4> cut_side_items(const std::vector<int>& counts, const std::vector<int64_t>& ptr, int64_t row_begin, int64_t row_end) {
  std::vector<int4> items;
  int64_t i = row_begin;
  while (i < row_end) {
    if (counts[(size_t)i] == 0) { ++i; continue; }
    int64_t j = i + 1;
    while (j < row_end && counts[(size_t)j] > 0 && ptr[(size_t)j + 1] - ptr[(size_t)i] <= 256 && j - i < 256) ++j;
    items.push_back(make_int4((int)ptr[(size_t)i], (int)ptr[(size_t)j], (int)i, (int)j));
    i = j;
  }
  return items;
}
// L2P work groups: a leaf of this tree holds ~19 panels, a third of a wavefront; consecutive leaves are packed until 64 rows or
// max_leaves (a leaf with more than 64 panels is a group of its own).  Group k: leaves [grp[k], grp[k + 1]); no leaves: {0, 0},
// which counts as no group.
inline std::vector<int> l2p_groups(const std::vector<int>& leaf_rows, int max_leaves) {
  std::vector<int> grp(1, 0);
  int rows = 0;
  for (size_t i = 0; i < leaf_rows.size(); ++i) {
    const int in_group = (int)i - grp.back();
    if (in_group > 0 && (rows + leaf_rows[i] > 64 || in_group == max_leaves)) { grp.push_back((int)i); rows = 0; }
    rows += leaf_rows[i];
  }
  grp.push_back((int)leaf_rows.size());
  return grp;
}
// items of the shifts: whole targets, ONE pass (at most 64 pairs) -- the shift kernels carry nothing between passes
inline void cut_single_pass(const std::vector<int>& seg_len, int pair_base, std::vector<int>& item_ptr, int lanes = 64) {
  item_ptr.push_back(pair_base);
  int fill = 0;
  for (int l : seg_len) {
    if (fill + l > lanes) { item_ptr.push_back(item_ptr.back() + fill); fill = 0; }
    fill += l;
  }
  if (fill > 0) item_ptr.push_back(item_ptr.back() + fill);
}

// ---------------------------------------- the near field ----------------------------------------
constexpr int64_t kNearItemBytes = 256 << 10;      // two-sphere N = 1M (near ms): 64 KB 0.81, 128 0.72, 192 0.74, 256 0.705, 320 0.735, 384 0.72, 512 0.72
constexpr int64_t kSymItemBytes = 512 << 10;       // red blood cell N = 524 288 (near ms): 128 KB 2.06-2.08, 256 KB 2.06-2.09, 512 KB 2.01-2.03

struct NearLayout {
  // leaves and the near block structure: runs of consecutive source rows per leaf (adjacent source leaves merged)
  std::vector<int> leaf_row0, leaf_nrows, near_stride, run_row0, run_off;
  std::vector<int64_t> near_off, run_ptr;
  int max_cols = 2, max_runs = 1;                   // widest row block / most runs of an owned leaf
  // hybrid near field (near_stream_fraction < 1): the leaves that keep no matrix
  bool hybrid = false;
  std::vector<uint8_t> rec;                         // [leaf] 1 = recomputed
  int64_t near_recomputed_pairs = 0;                // of the owned leaves
  // SpMV work items, largest first, and the pipelined kernel's records of the same items
  std::vector<int4> items;                          // (leaf, first row, rows, rows < 8)
  std::vector<NearItem> recs;
  // Stokes: the near blocks in their symmetric 6-value form, the only copy (stokes_sym off: the 9-value rows instead)
  bool stokes_sym = false;
  std::vector<int4> sym_items;
  std::vector<int64_t> sym_off;
  // float near field: the copy's offsets per leaf, and (Laplace) the item records again with the float rows' offsets and strides
  bool f32 = false;
  std::vector<int64_t> off32;
  std::vector<NearItem> recs32;
  // hybrid: the recompute items (panel rows) and their records
  std::vector<int4> rc_items;                       // (leaf, first row, rows, 0)
  std::vector<RcItem> rc_recs;
  int64_t near_total_doubles = 0, sym_total_doubles = 0, near_f32_floats = 0;     // what the flag side allocates
  int64_t near_bytes = 0;
};

inline std::vector<int4> pack_items(const std::vector<WorkItem>& items, bool colsplit) {
  std::vector<int4> packed(items.size());
  for (size_t i = 0; i < items.size(); ++i) packed[i] = make_int4(items[i].leaf, items[i].r0, items[i].nr, colsplit && items[i].nr < 8);
  return packed;
}

// Reads only what the host plan holds when HostOptions::after_near_lists fires: the tree, the leaves, the near lists, the shard's ranges
inline NearLayout near_layout(const HostPlan& hp, const LayoutOptions& o) {
  NearLayout L;
  const int nl = hp.nleaves(), dof = o.dof;
  L.leaf_row0.resize(nl); L.leaf_nrows.resize(nl); L.near_stride.resize(nl);
  L.near_off.assign(nl, 0); L.run_ptr.assign((size_t)nl + 1, 0); L.rec.assign(nl, 0);
  for (int l = 0; l < nl; ++l) {
    const int b = hp.leaf_box[l];
    L.leaf_nrows[l] = hp.box_body_end[b] - hp.box_body_begin[b];
  }
  // Hybrid near field: the leaves that keep NO matrix.  Chosen on the WHOLE tree (every shard builds the same tree and reaches the
  // same verdict for a leaf, so a shard's rows carry the bits of the single plan): the leaves with the most rows first -- a
  // recomputed pair costs the same arithmetic wherever it sits, but the source panel's 128 bytes are read once per item and
  // amortised over the item's rows -- until their pairs make up 1 - near_stream_fraction of all near pairs.
  {
    double f = o.near_stream_fraction;
    bool rule_ok = hp.rule.n <= (dof == 3 ? 4 : 3);               // the far-regime points of a source live in registers
    for (int q = 2; q < hp.rule.n; ++q) rule_ok = rule_ok && hp.rule.w[q] == hp.rule.w[1];      // K = 1, 3, 4: two distinct weights at most
    // runs of consecutive source rows per leaf (the pipelined kernels prefetch an item's run descriptors one per thread): counted
    // by the shares of a few threads, as the runs themselves are filled in below
    std::vector<int> nruns_of(nl, 0);
    int max_runs_owned = 1;
    parallel_rows(nl, 4096, [&](int64_t l0, int64_t l1) {
      for (int64_t l = l0; l < l1; ++l) {
        int c = 0;
        for (int64_t i = hp.near_ptr[l]; i < hp.near_ptr[l + 1]; ++i) c += i == hp.near_ptr[l] || hp.near_src[i - 1] + 1 != hp.near_src[i];
        nruns_of[l] = c;
      }
    });
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) max_runs_owned = std::max(max_runs_owned, nruns_of[l]);
    for (int l = 0; l < nl; ++l) L.run_ptr[l + 1] = L.run_ptr[l] + nruns_of[l];
    L.hybrid = f < 1.0 && o.sparse_local && hp.opt.evaluator == 0 && !o.treecode && rule_ok && (dof == 3 ? o.stokes_sym : near_pipe_ok(dof, max_runs_owned));
    if (L.hybrid) {
      if (!(f >= 0.0)) f = 0.0;
      std::vector<int> order(nl);
      for (int l = 0; l < nl; ++l) order[l] = l;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return L.leaf_nrows[a] > L.leaf_nrows[b]; });
      double all = 0;
      for (int l = 0; l < nl; ++l) all += (double)L.leaf_nrows[l] * hp.near_ncols[l];
      double acc = 0;
      for (int l : order) {
        if (acc >= (1.0 - f) * all) break;
        if (hp.near_ncols[l] > 8192) continue;        // a coarse leaf of an adaptive tree (10^4 columns): one item would run alone at the end
        if (nruns_of[l] > 256) continue;
        L.rec[l] = 1;
        acc += (double)L.leaf_nrows[l] * hp.near_ncols[l];
      }
      for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) if (L.rec[l]) L.near_recomputed_pairs += (int64_t)L.leaf_nrows[l] * hp.near_ncols[l];
    }
  }
  L.run_row0.resize((size_t)L.run_ptr[nl]); L.run_off.resize((size_t)L.run_ptr[nl]);
  parallel_rows(nl, 4096, [&](int64_t l0, int64_t l1) {
    for (int64_t l = l0; l < l1; ++l) {
      const int b = hp.leaf_box[l];
      L.leaf_row0[l] = hp.box_body_begin[b];
      L.near_stride[l] = (dof * hp.near_ncols[l] + 1) & ~1;      // in unknowns (dof per panel), rows 16-B aligned
      // source leaves are ascending; leaves with consecutive indices own adjacent rows -> one run
      int col = 0;
      int64_t k = L.run_ptr[l];
      for (int64_t i = hp.near_ptr[l]; i < hp.near_ptr[l + 1]; ++i) {
        const int sl = hp.near_src[i], sb = hp.leaf_box[sl];
        if (i == hp.near_ptr[l] || hp.near_src[i - 1] + 1 != sl) {
          L.run_row0[(size_t)k] = hp.box_body_begin[sb];
          L.run_off[(size_t)k] = col;
          ++k;
        }
        col += hp.box_body_end[sb] - hp.box_body_begin[sb];
      }
    }
  });
  int64_t total = 0;
  for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
    L.near_off[l] = total;
    if (!L.rec[l]) total += (int64_t)dof * L.leaf_nrows[l] * L.near_stride[l];
    L.max_cols = std::max(L.max_cols, L.near_stride[l]);
    L.max_runs = std::max(L.max_runs, (int)(L.run_ptr[l + 1] - L.run_ptr[l]));
  }
  auto nruns = [&](int l) { return (int)(L.run_ptr[l + 1] - L.run_ptr[l]); };
  {
    // SpMV work items: a leaf's row block, cut into row ranges of <= kNearItemBytes (two-sphere N=1M: one leaf is 58 rows x
    // 16 031 columns = 7.4 MB against a mean of 75 KB), dealt round-robin to the persistent workgroups largest first.
    // (a matrix-free plan runs the sweeps of kernels_near.hip over the same items, which count PANEL rows and pairs whatever
    // the number of unknowns per panel)
    std::vector<WorkItem> items;
    const int idof = o.sparse_local ? dof : 1;
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
      const int nr = idof * L.leaf_nrows[l];
      const int64_t row_bytes = o.sparse_local ? (int64_t)L.near_stride[l] * 8 : (int64_t)hp.near_ncols[l] * 8;
      if (nr == 0 || row_bytes == 0) continue;
      if (L.hybrid && (dof == 3 || L.rec[l])) continue;     // hybrid plans: Stokes builds its stream items below; a recomputed leaf has none
      cut_rows(l, nr, row_bytes, kNearItemBytes, items);
    }
    stable_sort_largest_first(items, [](const WorkItem& a) { return a.key; });
    L.items = pack_items(items, true);
    L.recs.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i) {
      const WorkItem& it = items[i];
      NearItem& q = L.recs[i];
      q.val_off = L.near_off[it.leaf] + (int64_t)it.r0 * L.near_stride[it.leaf];
      q.run_begin = L.run_ptr[it.leaf];
      q.nruns = nruns(it.leaf);
      q.yrow = dof * L.leaf_row0[it.leaf] + it.r0;
      q.nrows = it.nr;
      q.ncols = dof * hp.near_ncols[it.leaf];
      q.stride = L.near_stride[it.leaf];
      q.colsplit = it.nr < 8;
      q.pad[0] = q.pad[1] = 0;
    }
  }
  L.stokes_sym = dof == 3 && o.sparse_local && o.stokes_sym;
  L.near_total_doubles = (o.sparse_local && !L.stokes_sym) ? total : 0;      // matrix-free mode keeps no matrix
  L.near_bytes = L.near_total_doubles * (int64_t)sizeof(double);
  if (L.stokes_sym) {
    L.sym_off.assign(nl, 0);
    int64_t sym_total = 0;
    std::vector<WorkItem> items;
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
      const int nr = L.leaf_nrows[l], ncp = hp.near_ncols[l];
      L.sym_off[l] = sym_total;
      if (L.rec[l]) continue;                           // hybrid: no block, no stream item
      sym_total += (int64_t)6 * nr * ncp;
      if (nr == 0 || ncp == 0) continue;
      cut_rows(l, nr, (int64_t)48 * ncp, kSymItemBytes, items);
    }
    stable_sort_largest_first(items, [](const WorkItem& a) { return a.key; });
    L.sym_items = pack_items(items, true);
    L.sym_total_doubles = std::max<int64_t>(sym_total, 1);
    L.near_bytes = sym_total * (int64_t)sizeof(double);
  }
  // Float near field: the layout of the copy (device_plan.hpp near_f32) -- per leaf offsets, and for the pipelined Laplace kernel
  // the item records again with the offsets and strides of the float rows (recs itself is what the FP64 kernel reads).
  // The option's premise is that the rounding of the entries hides under the truncation error of the far field.  An FMM plan whose
  // leaves are ALL near one another (every leaf pair is a P2P pair: no M2L anywhere) has no far field: its result is exact at every
  // order, relaxation changes nothing, and there is nothing for the float error to hide under -- such a plan (a few hundred panels)
  // takes the option as 0.  The LOCAL / BLOCK_DIAGONAL evaluators are near-field operators by definition and keep it.
  const bool f32_premise = hp.opt.evaluator != 0 || hp.near_ptr[nl] < (int64_t)nl * nl;
  L.f32 = o.near_f32_max_p > 0 && o.sparse_local && !L.hybrid && !o.targets && hp.opt.shard_world <= 1 && L.near_bytes > 0 &&
          f32_premise && near_f32_ok(dof, L.max_runs, L.stokes_sym);
  if (L.f32) {
    L.off32.assign(nl, 0);
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
      L.off32[l] = L.near_f32_floats;
      L.near_f32_floats += dof == 3 ? (int64_t)12 * L.leaf_nrows[l] * ((hp.near_ncols[l] + 1) / 2) : (int64_t)L.leaf_nrows[l] * ((hp.near_ncols[l] + 3) & ~3);
    }
    if (dof == 1) {
      L.recs32 = L.recs;
      for (size_t i = 0; i < L.recs32.size(); ++i) {
        NearItem& q = L.recs32[i];
        const int l = L.items[i].x, s32 = (hp.near_ncols[l] + 3) & ~3;
        q.val_off = L.off32[l] + (q.val_off - L.near_off[l]) / L.near_stride[l] * s32;
        q.stride = s32;
      }
    }
  }
  if (L.hybrid) {
    // recompute items: ranges of <= 32 panel rows (Laplace: four wavefronts x eight) of the recomputed leaves; Stokes, sources
    // straight into LDS (near_recompute3g): a whole leaf of up to rcg_item_rows is one item -- its source panels are loaded once
    std::vector<WorkItem> items;
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
      const int nr = L.leaf_nrows[l], ncp = hp.near_ncols[l];
      if (!L.rec[l] || nr == 0 || ncp == 0) continue;
      cut_recompute(l, nr, ncp, dof == 3 ? o.rcg_item_rows : 32, items);
    }
    stable_sort_largest_first(items, [](const WorkItem& a) { return a.key; });
    L.rc_items = pack_items(items, false);
    L.rc_recs.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i) {
      const WorkItem& it = items[i];
      RcItem& q = L.rc_recs[i];
      q.prow0 = L.leaf_row0[it.leaf] + it.r0; q.nrows = it.nr; q.ncp = hp.near_ncols[it.leaf];
      q.run_begin = L.run_ptr[it.leaf]; q.nruns = nruns(it.leaf); q.leaf = it.leaf; q.pad = 0;
    }
  }
  return L;
}

// ---------------------------------------- the far field ----------------------------------------
// (first, items, pairs) of one level launch of the rotation kernels (kernels_m2l_rot.hip with FMMBEM_ROT_OP = 1, 2)
struct ShiftRot { int item_first = 0, n_items = 0, pairs = 0, level_boxes = 0, pair_first = 0, unit_first = 0, n_units = 0; };   // level_boxes: boxes of the child level in the WHOLE tree; units: parents (M2M) / pairs (L2L) of the one-pair-per-wavefront kernel

using LevelLaunches = std::vector<std::pair<int, int>>;          // (first, count) per level that holds anything

// one direction of the tree: the pairs (source box, class, target box) of all its launches, launch after launch, the rotation
// kernel's items (pair ranges of at most one pass), the class records and the wavefront kernel's class tables
struct SideLayout {
  std::vector<int> src, cls, tgt, item;
  std::vector<double> rec, sl_class;
  LevelLaunches launch;
  std::vector<ShiftRot> rot;
};

struct FarLayout {
  std::vector<int> p2m_leaf, l2p_leaf, l2p_grp;
  int n_l2p_grp = 0;
  bool l2p_scatter = false;                           // L2P's groups cover every row of a Laplace plan on its own panels, one shard
  SideLayout up, down;                                // M2M / L2L
  std::vector<int> up_unit_ptr;                       // first pair of every parent, per launch
  LevelLaunches shared_launch;                        // sharded upward pass: parents spanning shards (pairs and items in `up`)
  std::vector<ShiftRot> shared_rot;
  std::vector<int> up_cls, down_cls;                  // [box] class of (parent - box)
  std::vector<tables::cplx> up_tab, down_tab;         // [class][p_max^2]
  std::vector<int> m2l_tgt, mh_box;                   // targets to run; sources whose Mh is needed
  std::vector<int> m2p_chain_ptr, m2p_chain_box, m2p_item_leaf, m2p_item_row;     // treecode plans only
  int64_t n_classes = 0;
  int g_max = 0;
  std::vector<double> m2l_g;                          // [class][g_max]
  std::vector<tables::cplx> m2l_z;                    // [class][p_max]
  std::vector<double> rot_cls_rec;                    // [class][8]
};

inline LevelLaunches level_launches(const std::vector<int>& ptr) {
  LevelLaunches out;
  for (size_t l = 0; l + 1 < ptr.size(); ++l)
    if (ptr[l + 1] > ptr[l]) out.emplace_back(ptr[l], ptr[l + 1] - ptr[l]);
  return out;
}

inline FarLayout far_layout(const HostPlan& hp, const tables::HarmonicTables& T, const LayoutOptions& o) {
  using namespace tables;
  FarLayout F;
  const int nb = hp.nboxes, pm = hp.opt.p_max;
  auto leaf_rows = [&](int lf) { return hp.box_body_end[hp.leaf_box[lf]] - hp.box_body_begin[hp.leaf_box[lf]]; };
  for (int b : hp.p2m_leaves) F.p2m_leaf.push_back(hp.box_leaf_index[b]);
  for (int b : hp.l2p_leaves) F.l2p_leaf.push_back(hp.box_leaf_index[b]);
  {
    std::vector<int> rows(F.l2p_leaf.size());
    int64_t covered = 0;                               // the L2P leaves are distinct leaves: all rows are theirs when the counts agree
    for (size_t i = 0; i < rows.size(); ++i) covered += rows[i] = leaf_rows(F.l2p_leaf[i]);
    F.l2p_grp = l2p_groups(rows, o.l2p_group_leaves);
    F.n_l2p_grp = F.l2p_leaf.empty() ? 0 : (int)F.l2p_grp.size() - 1;
    F.l2p_scatter = o.dof == 1 && !o.targets && hp.opt.shard_world <= 1 && !F.l2p_leaf.empty() && covered == (int64_t)hp.n;
  }
  F.up.launch = level_launches(hp.m2m_level_ptr); F.down.launch = level_launches(hp.l2l_level_ptr); F.shared_launch = level_launches(hp.m2m_shared_ptr);
  // parent<->child translation classes, their regular-harmonic tables and their records for the rotation kernels
  {
    F.up_cls.assign(nb, 0); F.down_cls.assign(nb, 0);
    std::unordered_map<IVec3, int, IVec3Hash> seen;
    std::vector<cplx> h;
    for (int b = 1; b < nb; ++b) {
      const int par = hp.box_parent[b];
      const int32_t v[3] = {hp.box_icoord[3 * par] - hp.box_icoord[3 * b], hp.box_icoord[3 * par + 1] - hp.box_icoord[3 * b + 1],
                            hp.box_icoord[3 * par + 2] - hp.box_icoord[3 * b + 2]};
      auto [it, fresh] = seen.try_emplace(IVec3{v[0], v[1], v[2]}, (int)seen.size());
      if (fresh) {
        double up[3], down[3];
        for (int k = 0; k < 3; ++k) { up[k] = 0.5 * hp.cell[k] * double(v[k]); down[k] = -up[k]; }
        F.up.rec.resize(F.up.rec.size() + 8); F.down.rec.resize(F.down.rec.size() + 8);
        rot_record(up, F.up.rec.data() + F.up.rec.size() - 8); rot_record(down, F.down.rec.data() + F.down.rec.size() - 8);
        shift_class_table(T, up, true, pm, h, F.up_tab);          // M2M: of (parent - child)
        shift_class_table(T, down, false, pm, h, F.down_tab);     // L2L: of (child - parent)
      }
      F.up_cls[b] = F.down_cls[b] = it->second;
    }
  }
  // ---- M2M / L2L by rotation: pair lists per level launch, items ----
  {
    std::vector<int> len;
    auto level_boxes = [&](int l) { return l >= 0 && l < hp.nlevels ? hp.level_off[l + 1] - hp.level_off[l] : 0; };
    // The pairs of a side's launches, launch after launch, with each launch's items and ShiftRot.  unit(i) appends the pairs of
    // entry i of the side's box list and returns the level of their CHILD boxes; uptr: the wavefront kernel walks a unit's
    // pairs through it (M2M: a parent's children), null: a pair is a unit (L2L)
    auto add_launches = [&](SideLayout& sd, const LevelLaunches& launches, std::vector<ShiftRot>& out, std::vector<int>* uptr, auto&& unit) {
      for (auto [first, count] : launches) {
        ShiftRot sr;
        sr.item_first = (int)sd.item.size();
        const int base = sr.pair_first = (int)sd.src.size();
        if (uptr) sr.unit_first = (int)uptr->size();
        sr.n_units = count;
        len.clear();
        for (int i = first; i < first + count; ++i) {
          const int before = (int)sd.src.size();
          if (uptr) uptr->push_back(before);
          const int child_level = unit(i);
          if (i == first) sr.level_boxes = level_boxes(child_level);
          len.push_back((int)sd.src.size() - before);
        }
        if (uptr) uptr->push_back((int)sd.src.size());    // one past the level's last parent
        cut_single_pass(len, base, sd.item);
        sr.n_items = (int)sd.item.size() - sr.item_first - 1;
        sr.pairs = (int)sd.src.size() - base;
        out.push_back(sr);
      }
    };
    auto m2m_unit = [&](int i) {
      const int par = hp.m2m_parents[i];
      for (int c = hp.box_child_begin[par]; c < hp.box_child_end[par]; ++c) { F.up.src.push_back(c); F.up.cls.push_back(F.up_cls[c]); F.up.tgt.push_back(par); }
      return hp.box_level[par] + 1;
    };
    add_launches(F.up, F.up.launch, F.up.rot, &F.up_unit_ptr, m2m_unit);
    add_launches(F.up, F.shared_launch, F.shared_rot, &F.up_unit_ptr, m2m_unit);
    add_launches(F.down, F.down.launch, F.down.rot, nullptr, [&](int i) {
      const int c = hp.l2l_children[i];
      F.down.src.push_back(hp.box_parent[c]); F.down.cls.push_back(F.down_cls[c]); F.down.tgt.push_back(c);
      return hp.box_level[c];
    });
    // one pair per wavefront: class tables
    const int nclass = (int)F.up.rec.size() / 8, cs = sl_class_doubles(pm);
    F.up.sl_class.resize((size_t)nclass * cs); F.down.sl_class.resize((size_t)nclass * cs);
    for (int c = 0; c < nclass; ++c) {
      sl_class_table(F.up.rec.data() + (size_t)c * 8, pm, kRotM2M, F.up.sl_class.data() + (size_t)c * cs);
      sl_class_table(F.down.rec.data() + (size_t)c * 8, pm, kRotL2L, F.down.sl_class.data() + (size_t)c * cs);
    }
  }
  // M2L: targets to run, sources whose Mh is needed
  {
    std::vector<uint8_t> is_src(nb, 0);
    for (int b = 0; b < nb; ++b)
      if (hp.has_L[b] && hp.owned_L[b]) F.m2l_tgt.push_back(b);
    for (int s : hp.m2l_src) is_src[s] = 1;
    for (int b = 0; b < nb; ++b) if (is_src[b]) F.mh_box.push_back(b);
  }
  if (o.treecode) {
    // M2P work (device_launch.hpp M2PWork): per leaf the boxes of its path that are the target of a pair, root first -- box_parent
    // is read here and never on the device -- and the leaves that have any cut into items of up to 64 rows
    std::vector<int> path;
    F.m2p_chain_ptr.assign((size_t)hp.nleaves() + 1, 0);
    for (int l = 0; l < hp.nleaves(); ++l) {
      path.clear();
      for (int b = hp.leaf_box[l]; b >= 0; b = b > 0 ? hp.box_parent[b] : -1)
        if (hp.m2l_ptr[b + 1] > hp.m2l_ptr[b]) path.push_back(b);
      F.m2p_chain_box.insert(F.m2p_chain_box.end(), path.rbegin(), path.rend());
      F.m2p_chain_ptr[l + 1] = (int)F.m2p_chain_box.size();
      const int nr = leaf_rows(l);
      for (int r = 0; r < nr && !path.empty(); r += 64) { F.m2p_item_leaf.push_back(l); F.m2p_item_row.push_back(r); }
    }
  }
  // M2L class tables and the rotation kernel's class records.  The translation = c_target - c_source (executor/M2L.hpp:40) is
  // rebuilt from the exact integer class vector (half-cell units) so that a table does not depend on which pair was seen first
  // (shards of one operator must produce bit-identical rows).
  F.n_classes = (int64_t)hp.m2l_class_rep.size() / 2;
  F.g_max = m2l_entries(pm);
  F.m2l_g.resize((size_t)F.n_classes * F.g_max);
  F.m2l_z.resize((size_t)F.n_classes * pm);
  F.rot_cls_rec.assign((size_t)F.n_classes * 8, 0.0);
  parallel_rows(F.n_classes, 64, [&](int64_t c_begin, int64_t c_end) {
    std::vector<cplx> h;
    for (int64_t c = c_begin; c < c_end; ++c) {
      double tr[3];
      for (int k = 0; k < 3; ++k) tr[k] = 0.5 * hp.cell[k] * double(hp.m2l_class_vec[3 * c + k]);
      m2l_class_rows(T, tr, pm, h, F.m2l_g.data() + (size_t)c * F.g_max, F.m2l_z.data() + (size_t)c * pm);
      rot_record(tr, F.rot_cls_rec.data() + (size_t)c * 8);
    }
  });
  return F;
}

}  // namespace fmmbem
