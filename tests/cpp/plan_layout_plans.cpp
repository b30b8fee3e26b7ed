// plan_layout_plans.cpp -- host-only program of tests/test_plan_layout_host.py: builds a real HostPlan (csrc/host_plan.cpp) from a
// mesh file, runs near_layout inside HostOptions::after_near_lists (where plan.hip runs it) and far_layout after the build, and checks
// the STRUCTURE of what they return against the host plan -- coverage, order, partitions, contiguity -- never against values the
// layouts computed themselves.  Prints one "FAIL ..." line per broken property and a summary line.  Built with plain g++.
//   plan_layout_plans mesh.bin ncrit [key=value ...]     keys: kernel sym sparse f f32 tree rank world upward targets
#include <algorithm>
#include <array>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../fmm-bem-relaxed_amd/csrc/plan_layout.hpp"

using namespace fmmbem;
using namespace fmmbem::tables;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                   \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (g_fail++ < 20) { std::printf("FAIL line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                                      \
  } while (0)

template <class T>
static std::vector<T> read_vec(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::printf("FAIL short file\n"); std::exit(2); }
  return v;
}

static int rows_of(const HostPlan& hp, int l) { return hp.box_body_end[hp.leaf_box[l]] - hp.box_body_begin[hp.leaf_box[l]]; }

// every row [0, rows(l)) of the leaves `want` says in exactly one item, every other leaf in none; largest first, ties in (leaf, row) order
template <class Rows, class Key>
static void check_items(const char* what, const HostPlan& hp, const std::vector<int4>& items, Rows&& want_rows, Key&& key, bool colsplit) {
  std::vector<std::vector<std::pair<int, int>>> by_leaf(hp.nleaves());
  for (size_t i = 0; i < items.size(); ++i) {
    const int4 it = items[i];
    CHECK(it.x >= hp.leaf_begin && it.x < hp.leaf_end, "%s item %zu leaf %d", what, i, it.x);
    if (it.x < 0 || it.x >= hp.nleaves()) continue;
    CHECK(it.z > 0 && it.w == (colsplit && it.z < 8), "%s item %zu", what, i);
    by_leaf[it.x].push_back({it.y, it.z});
    if (i > 0) {
      const int4 pv = items[i - 1];
      const int64_t ka = key(pv), kb = key(it);
      CHECK(ka >= kb, "%s items %zu, %zu grow: %lld < %lld", what, i - 1, i, (long long)ka, (long long)kb);
      if (ka == kb) CHECK(pv.x < it.x || (pv.x == it.x && pv.y < it.y), "%s equal items %zu, %zu out of leaf / row order", what, i - 1, i);
    }
  }
  for (int l = 0; l < hp.nleaves(); ++l) {
    const int want = l >= hp.leaf_begin && l < hp.leaf_end ? want_rows(l) : 0;
    std::sort(by_leaf[l].begin(), by_leaf[l].end());
    int at = 0;
    for (auto [r0, nr] : by_leaf[l]) { CHECK(r0 == at, "%s leaf %d: row %d covered %s", what, l, at, r0 < at ? "twice" : "by no item"); at = r0 + nr; }
    CHECK(at == want, "%s leaf %d: %d of %d rows in items", what, l, at, want);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::map<std::string, std::string> kv;
  for (int i = 3; i < argc; ++i) { const char* eq = std::strchr(argv[i], '='); if (eq) kv[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1; }
  auto geti = [&](const char* k, int dflt) { return kv.count(k) ? std::atoi(kv[k].c_str()) : dflt; };
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const int64_t n = read_vec<int64_t>(f, 1)[0];
  const std::vector<double> vertices = read_vec<double>(f, (size_t)n * 9);
  const std::vector<uint8_t> bc = read_vec<uint8_t>(f, (size_t)n);
  std::fclose(f);

  LayoutOptions o;
  const bool stokes = geti("kernel", 0) == 1;
  o.dof = stokes ? 3 : 1;
  o.sparse_local = geti("sparse", 1) != 0;
  o.treecode = geti("tree", 0) != 0;
  o.targets = kv.count("targets") != 0;
  o.near_stream_fraction = kv.count("f") ? std::atof(kv["f"].c_str()) : 1.0;
  o.stokes_sym = geti("sym", 1) != 0;
  o.near_f32_max_p = geti("f32", 0);
  o.rcg_item_rows = 60;
  o.l2p_group_leaves = stokes ? 4 : 8;
  HostOptions ho;
  ho.p_max = 8; ho.quad_k = stokes ? 4 : 3; ho.ncrit = (unsigned)std::atoi(argv[2]);
  ho.shard_rank = geti("rank", 0); ho.shard_world = geti("world", 1); ho.shard_upward = geti("upward", 0);
  ho.panels_on_device = true;

  HostPlan hp;
  NearLayout L;
  bool hook = false;
  std::string err;
  if (o.targets) {
    FILE* g = std::fopen(kv["targets"].c_str(), "rb");
    if (!g) return 2;
    const int64_t m = read_vec<int64_t>(g, 1)[0];
    const std::vector<double> pts = read_vec<double>(g, (size_t)m * 3);
    const std::vector<uint8_t> tbc = read_vec<uint8_t>(g, (size_t)m);
    std::fclose(g);
    ho.panels_on_device = false;
    err = hp.build_targets(ho, n, vertices.data(), m, pts.data(), tbc.data());
    if (err.empty()) L = near_layout(hp, o);
  } else {
    // as fmmbem_plan_create: the near layout is made while the host plan is still without its far-field lists
    ho.after_near_lists = [&]() -> std::string { L = near_layout(hp, o); hook = true; return std::string(); };
    err = hp.build(ho, n, vertices.data(), bc.data());
    CHECK(hook, "after_near_lists did not fire");
  }
  if (!err.empty()) { std::printf("FAIL build: %s\n", err.c_str()); return 1; }
  const HarmonicTables T;
  const FarLayout F = far_layout(hp, T, o);
  const int nl = hp.nleaves(), nb = hp.nboxes, dof = o.dof, pm = hp.opt.p_max;
  auto owned = [&](int l) { return l >= hp.leaf_begin && l < hp.leaf_end; };

  // ---- the near field ----
  // the runs of a leaf expand to exactly the rows of its near_src leaves, in order
  int max_runs = 1;
  for (int l = 0; l < nl; ++l) {
    std::vector<int> want, got;
    for (int64_t i = hp.near_ptr[l]; i < hp.near_ptr[l + 1]; ++i) {
      const int sb = hp.leaf_box[hp.near_src[i]];
      for (int r = hp.box_body_begin[sb]; r < hp.box_body_end[sb]; ++r) want.push_back(r);
    }
    CHECK((int)want.size() == hp.near_ncols[l], "leaf %d", l);
    for (int64_t k = L.run_ptr[l]; k < L.run_ptr[l + 1]; ++k) {
      const int end = k + 1 < L.run_ptr[l + 1] ? L.run_off[(size_t)k + 1] : hp.near_ncols[l];
      CHECK(L.run_off[(size_t)k] == (int)got.size() && end > L.run_off[(size_t)k], "leaf %d run %lld", l, (long long)k);
      if (k > L.run_ptr[l]) CHECK(L.run_row0[(size_t)k] != L.run_row0[(size_t)k - 1] + (L.run_off[(size_t)k] - L.run_off[(size_t)k - 1]), "leaf %d: runs %lld and the one before are one run", l, (long long)k);
      for (int c = L.run_off[(size_t)k]; c < end; ++c) got.push_back(L.run_row0[(size_t)k] + (c - L.run_off[(size_t)k]));
    }
    CHECK(got == want, "leaf %d: the runs do not expand to the rows of near_src", l);
    CHECK(L.leaf_row0[l] == hp.box_body_begin[hp.leaf_box[l]] && L.leaf_nrows[l] == rows_of(hp, l), "leaf %d", l);
    CHECK(L.near_stride[l] >= dof * hp.near_ncols[l] && L.near_stride[l] <= dof * hp.near_ncols[l] + 1 && L.near_stride[l] % 2 == 0, "leaf %d stride", l);
    if (owned(l)) max_runs = std::max(max_runs, (int)(L.run_ptr[l + 1] - L.run_ptr[l]));
  }
  CHECK(L.max_runs == max_runs, "%d %d", L.max_runs, max_runs);
  // block offsets are contiguous over the owned leaves, a recomputed leaf holds nothing, and the totals match
  {
    int64_t at = 0, at_sym = 0, at32 = 0, rec_pairs = 0;
    int max_cols = 2;
    for (int l = hp.leaf_begin; l < hp.leaf_end; ++l) {
      CHECK(L.near_off[l] == at, "leaf %d near_off", l);
      if (!L.rec[l]) at += (int64_t)dof * rows_of(hp, l) * L.near_stride[l];
      else rec_pairs += (int64_t)rows_of(hp, l) * hp.near_ncols[l];
      max_cols = std::max(max_cols, L.near_stride[l]);
      if (L.stokes_sym) { CHECK(L.sym_off[l] == at_sym, "leaf %d sym_off", l); if (!L.rec[l]) at_sym += (int64_t)6 * rows_of(hp, l) * hp.near_ncols[l]; }
      if (L.f32) { CHECK(L.off32[l] == at32, "leaf %d off32", l); at32 += dof == 3 ? (int64_t)12 * rows_of(hp, l) * ((hp.near_ncols[l] + 1) / 2) : (int64_t)rows_of(hp, l) * ((hp.near_ncols[l] + 3) / 4 * 4); }
    }
    CHECK(L.max_cols == max_cols, "%d %d", L.max_cols, max_cols);
    CHECK(L.near_recomputed_pairs == rec_pairs, "recomputed pairs");
    CHECK(L.stokes_sym == (stokes && o.sparse_local && o.stokes_sym), "stokes_sym");
    CHECK(L.near_total_doubles == (o.sparse_local && !L.stokes_sym ? at : 0), "near_total_doubles");
    CHECK(L.sym_total_doubles == (L.stokes_sym ? std::max<int64_t>(at_sym, 1) : 0), "sym_total_doubles");
    CHECK(L.near_bytes == 8 * (L.stokes_sym ? at_sym : L.near_total_doubles), "near_bytes");
    CHECK(L.near_f32_floats == at32, "near_f32_floats");
  }
  // every owned row of a leaf that keeps its matrix lies in exactly one item, a recomputed leaf in none (and in the recompute items)
  const int idof = o.sparse_local ? dof : 1;
  auto row_bytes = [&](int l) { return o.sparse_local ? (int64_t)L.near_stride[l] * 8 : (int64_t)hp.near_ncols[l] * 8; };
  check_items("near", hp, L.items,
              [&](int l) { return (L.hybrid && (dof == 3 || L.rec[l])) || hp.near_ncols[l] == 0 ? 0 : idof * rows_of(hp, l); },
              [&](const int4& it) { return it.z * row_bytes(it.x); }, true);
  check_items("sym", hp, L.sym_items, [&](int l) { return !L.stokes_sym || L.rec[l] || hp.near_ncols[l] == 0 ? 0 : rows_of(hp, l); },
              [&](const int4& it) { return (int64_t)it.z * 48 * hp.near_ncols[it.x]; }, true);
  check_items("recompute", hp, L.rc_items, [&](int l) { return L.hybrid && L.rec[l] && hp.near_ncols[l] > 0 ? rows_of(hp, l) : 0; },
              [&](const int4& it) { return (int64_t)it.z * hp.near_ncols[it.x]; }, false);
  for (const int4& it : L.items) CHECK(it.z * row_bytes(it.x) <= kNearItemBytes || it.z <= 4, "near item of %d rows, %lld bytes", it.z, (long long)(it.z * row_bytes(it.x)));
  for (const int4& it : L.rc_items) CHECK(it.z <= (dof == 3 ? o.rcg_item_rows : 32), "recompute item of %d rows", it.z);
  // each record says what its leaf's offset, stride and runs imply
  CHECK(L.recs.size() == L.items.size() && L.rc_recs.size() == L.rc_items.size(), "record counts");
  for (size_t i = 0; i < L.recs.size() && i < L.items.size(); ++i) {
    const int4 it = L.items[i];
    const NearItem& q = L.recs[i];
    CHECK(q.val_off == L.near_off[it.x] + (int64_t)it.y * L.near_stride[it.x] && q.run_begin == L.run_ptr[it.x] &&
          q.nruns == (int)(L.run_ptr[it.x + 1] - L.run_ptr[it.x]) && q.yrow == dof * L.leaf_row0[it.x] + it.y && q.nrows == it.z &&
          q.ncols == dof * hp.near_ncols[it.x] && q.stride == L.near_stride[it.x] && q.colsplit == it.w && q.pad[0] == 0 && q.pad[1] == 0, "record %zu", i);
  }
  for (size_t i = 0; i < L.rc_recs.size() && i < L.rc_items.size(); ++i) {
    const int4 it = L.rc_items[i];
    const RcItem& q = L.rc_recs[i];
    CHECK(q.prow0 == L.leaf_row0[it.x] + it.y && q.nrows == it.z && q.ncp == hp.near_ncols[it.x] && q.run_begin == L.run_ptr[it.x] &&
          q.nruns == (int)(L.run_ptr[it.x + 1] - L.run_ptr[it.x]) && q.leaf == it.x && q.pad == 0, "recompute record %zu", i);
  }
  // a float record addresses the same rows as its FP64 twin, in the float copy's layout
  CHECK(L.recs32.size() == (L.f32 && dof == 1 ? L.recs.size() : 0), "float records");
  for (size_t i = 0; i < L.recs32.size(); ++i) {
    const NearItem &q = L.recs32[i], &t = L.recs[i];
    const int l = L.items[i].x, s32 = (hp.near_ncols[l] + 3) / 4 * 4;
    CHECK(q.val_off == L.off32[l] + (int64_t)L.items[i].y * s32 && q.stride == s32 && q.run_begin == t.run_begin && q.nruns == t.nruns &&
          q.yrow == t.yrow && q.nrows == t.nrows && q.ncols == t.ncols && q.colsplit == t.colsplit, "float record %zu", i);
  }
  // the hybrid choice, on the whole tree: the leaves with the most rows first, none above 8 192 columns or 256 runs, until they
  // hold 1 - f of the pairs (or no leaf is left to take)
  uint64_t rec_hash = 1469598103934665603ull;
  {
    double all = 0, chosen = 0;
    int least_chosen = INT32_MAX, most_left = 0, n_rec = 0;
    for (int l = 0; l < nl; ++l) {
      const double pairs = (double)rows_of(hp, l) * hp.near_ncols[l];
      const int runs = (int)(L.run_ptr[l + 1] - L.run_ptr[l]);
      all += pairs;
      rec_hash = (rec_hash ^ L.rec[l]) * 1099511628211ull;
      if (L.rec[l]) {
        ++n_rec; chosen += pairs; least_chosen = std::min(least_chosen, rows_of(hp, l));
        CHECK(L.hybrid && hp.near_ncols[l] <= 8192 && runs <= 256, "recomputed leaf %d", l);
      } else if (hp.near_ncols[l] <= 8192 && runs <= 256) most_left = std::max(most_left, rows_of(hp, l));
    }
    if (L.hybrid) {
      const double f = std::max(0.0, o.near_stream_fraction);
      CHECK(chosen >= (1.0 - f) * all || most_left == 0, "the recomputed leaves hold %.0f of %.0f pairs", chosen, all);
      CHECK(most_left <= least_chosen, "a leaf of %d rows was passed over for one of %d", most_left, least_chosen);
    }
    std::printf("hybrid %d leaves %d recomputed %d hash %llx\n", (int)L.hybrid, nl, n_rec, (unsigned long long)rec_hash);
  }

  // ---- the far field ----
  // L2P groups: a partition of the list, at most 64 rows (one leaf may have more) and max_leaves leaves each
  {
    CHECK(F.l2p_leaf.size() == hp.l2p_leaves.size() && F.p2m_leaf.size() == hp.p2m_leaves.size(), "leaf lists");
    const int ng = F.n_l2p_grp;
    CHECK((int)F.l2p_grp.size() >= ng + 1 && F.l2p_grp[0] == 0 && F.l2p_grp[ng] == (int)F.l2p_leaf.size(), "groups");
    CHECK((ng == 0) == F.l2p_leaf.empty(), "groups of an empty list");
    std::set<int> distinct(F.l2p_leaf.begin(), F.l2p_leaf.end());
    int64_t covered = 0;
    for (int lf : distinct) covered += rows_of(hp, lf);
    for (int k = 0; k < ng; ++k) {
      const int a = F.l2p_grp[k], b = F.l2p_grp[k + 1];
      int rows = 0;
      for (int i = a; i < b; ++i) { rows += rows_of(hp, F.l2p_leaf[i]); CHECK(hp.leaf_box[F.l2p_leaf[i]] == hp.l2p_leaves[i], "l2p leaf %d", i); }
      CHECK(b > a && b - a <= o.l2p_group_leaves && (rows <= 64 || b - a == 1), "group %d: leaves [%d, %d), %d rows", k, a, b, rows);
      // greedy: the next leaf did not fit
      if (k + 1 < ng) CHECK(b - a == o.l2p_group_leaves || rows + rows_of(hp, F.l2p_leaf[b]) > 64, "group %d closed early", k);
    }
    const bool expect = dof == 1 && !o.targets && hp.opt.shard_world <= 1 && !F.l2p_leaf.empty() && distinct.size() == F.l2p_leaf.size() && covered == hp.n;
    CHECK(F.l2p_scatter == expect, "l2p_scatter %d, rows covered %lld of %lld", (int)F.l2p_scatter, (long long)covered, (long long)hp.n);
    std::printf("l2p groups %d scatter %d\n", ng, (int)F.l2p_scatter);
  }
  // the classes of the tree passes: boxes with the same (parent - box) vector share one, and its record is that vector's
  {
    const int nclass = (int)F.up.rec.size() / 8;
    std::map<std::vector<int>, int> seen;
    for (int b = 1; b < nb; ++b) {
      const int par = hp.box_parent[b];
      std::vector<int> v(3);
      double up[3], down[3], r8[8];
      for (int k = 0; k < 3; ++k) { v[k] = hp.box_icoord[3 * par + k] - hp.box_icoord[3 * b + k]; up[k] = 0.5 * hp.cell[k] * v[k]; down[k] = -up[k]; }
      auto it = seen.emplace(v, F.up_cls[b]).first;
      CHECK(it->second == F.up_cls[b] && F.down_cls[b] == F.up_cls[b] && F.up_cls[b] >= 0 && F.up_cls[b] < nclass, "class of box %d", b);
      if (F.up_cls[b] < 0 || F.up_cls[b] >= nclass) continue;
      rot_record(up, r8);
      CHECK(std::memcmp(r8, F.up.rec.data() + 8 * F.up_cls[b], sizeof(r8)) == 0, "up record of box %d", b);
      rot_record(down, r8);
      CHECK(std::memcmp(r8, F.down.rec.data() + 8 * F.down_cls[b], sizeof(r8)) == 0, "down record of box %d", b);
    }
    CHECK((int)seen.size() == nclass && F.down.rec.size() == F.up.rec.size(), "classes");
    CHECK(F.up_tab.size() == (size_t)nclass * pm * pm && F.down_tab.size() == F.up_tab.size(), "shift tables");
    CHECK(F.up.sl_class.size() == (size_t)nclass * sl_class_doubles(pm) && F.down.sl_class.size() == F.up.sl_class.size(), "wavefront class tables");
  }
  // each launch's pairs, unit pointers and items partition its level
  {
    auto level_boxes = [&](int l) { return l >= 0 && l < hp.nlevels ? hp.level_off[l + 1] - hp.level_off[l] : 0; };
    auto check_side = [&](const char* what, const SideLayout& sd, const LevelLaunches& launches, const std::vector<ShiftRot>& rots,
                          const std::vector<int>& level_ptr, const std::vector<int>* uptr, int& pair_at, int& item_at, int& unit_at, auto&& unit_pairs) {
      size_t li = 0;
      for (size_t lv = 0; lv + 1 < level_ptr.size(); ++lv) {
        const int first = level_ptr[lv], count = level_ptr[lv + 1] - first;
        if (count <= 0) continue;
        CHECK(li < launches.size() && li < rots.size(), "%s: level %zu has no launch", what, lv);
        if (li >= launches.size() || li >= rots.size()) break;
        const ShiftRot& sr = rots[li];
        CHECK(launches[li].first == first && launches[li].second == count && sr.n_units == count, "%s launch %zu", what, li);
        CHECK(sr.pair_first == pair_at && sr.item_first == item_at && (!uptr || sr.unit_first == unit_at), "%s launch %zu starts", what, li);
        std::set<int> unit_starts;
        int at = pair_at;
        for (int u = 0; u < count; ++u) {
          unit_starts.insert(at);
          if (uptr) CHECK((*uptr)[unit_at + u] == at, "%s launch %zu unit %d", what, li, u);
          std::vector<std::array<int, 3>> want;
          const int child_level = unit_pairs(first + u, want);
          if (u == 0) CHECK(sr.level_boxes == level_boxes(child_level), "%s launch %zu level_boxes", what, li);
          for (const auto& w : want) {
            CHECK(at < (int)sd.src.size() && sd.src[at] == w[0] && sd.cls[at] == w[1] && sd.tgt[at] == w[2], "%s pair %d", what, at);
            ++at;
          }
        }
        unit_starts.insert(at);
        if (uptr) { CHECK((*uptr)[unit_at + count] == at, "%s launch %zu last unit", what, li); unit_at += count + 1; }
        CHECK(sr.pairs == at - pair_at, "%s launch %zu pairs", what, li);
        // the items: whole units, at most 64 pairs, from the launch's first pair to its last
        CHECK(sd.item[item_at] == pair_at && sd.item[item_at + sr.n_items] == at, "%s launch %zu items", what, li);
        for (int k = 0; k < sr.n_items; ++k) {
          const int a = sd.item[item_at + k], b = sd.item[item_at + k + 1];
          CHECK(b > a && b - a <= 64 && unit_starts.count(a) && unit_starts.count(b), "%s launch %zu item %d: pairs [%d, %d)", what, li, k, a, b);
        }
        item_at += sr.n_items + 1;
        pair_at = at;
        ++li;
      }
      CHECK(li == launches.size() && li == rots.size(), "%s: launches", what);
    };
    auto m2m_pairs = [&](int i, std::vector<std::array<int, 3>>& want) {
      const int par = hp.m2m_parents[i];
      for (int c = hp.box_child_begin[par]; c < hp.box_child_end[par]; ++c) want.push_back({c, F.up_cls[c], par});
      return hp.box_level[par] + 1;
    };
    int pair_at = 0, item_at = 0, unit_at = 0;
    check_side("up", F.up, F.up.launch, F.up.rot, hp.m2m_level_ptr, &F.up_unit_ptr, pair_at, item_at, unit_at, m2m_pairs);
    check_side("up shared", F.up, F.shared_launch, F.shared_rot, hp.m2m_shared_ptr, &F.up_unit_ptr, pair_at, item_at, unit_at, m2m_pairs);
    CHECK(pair_at == (int)F.up.src.size() && item_at == (int)F.up.item.size() && unit_at == (int)F.up_unit_ptr.size(), "up: nothing beyond the launches");
    int up_pairs = pair_at;
    pair_at = item_at = unit_at = 0;
    check_side("down", F.down, F.down.launch, F.down.rot, hp.l2l_level_ptr, nullptr, pair_at, item_at, unit_at, [&](int i, std::vector<std::array<int, 3>>& want) {
      const int c = hp.l2l_children[i];
      want.push_back({hp.box_parent[c], F.down_cls[c], c});
      return hp.box_level[c];
    });
    CHECK(pair_at == (int)F.down.src.size() && item_at == (int)F.down.item.size(), "down: nothing beyond the launches");
    std::printf("shift pairs up %d down %d shared launches %zu\n", up_pairs, pair_at, F.shared_launch.size());
  }
  // M2L: the owned boxes that hold an L, the distinct sources, one row per class
  {
    std::set<int> src(hp.m2l_src.begin(), hp.m2l_src.end());
    CHECK(std::vector<int>(src.begin(), src.end()) == F.mh_box, "Mh boxes");
    std::vector<int> tgt;
    for (int b = 0; b < nb; ++b) if (hp.has_L[b] && hp.owned_L[b]) tgt.push_back(b);
    CHECK(tgt == F.m2l_tgt, "M2L targets");
    CHECK(F.n_classes == (int64_t)hp.m2l_class_vec.size() / 3 && F.g_max == pm * (2 * pm + 1), "classes");
    CHECK(F.m2l_g.size() == (size_t)F.n_classes * F.g_max && F.m2l_z.size() == (size_t)F.n_classes * pm && F.rot_cls_rec.size() == (size_t)F.n_classes * 8, "class tables");
    for (int64_t c = 0; c < F.n_classes && F.rot_cls_rec.size() == (size_t)F.n_classes * 8; ++c) {
      double tr[3], r8[8];
      for (int k = 0; k < 3; ++k) tr[k] = 0.5 * hp.cell[k] * hp.m2l_class_vec[3 * c + k];
      rot_record(tr, r8);
      CHECK(std::memcmp(r8, F.rot_cls_rec.data() + 8 * c, sizeof(r8)) == 0, "record of class %lld", (long long)c);
    }
  }
  // M2P chains: the boxes of the leaf's path that are the target of a pair, root first
  if (o.treecode) {
    CHECK((int)F.m2p_chain_ptr.size() == nl + 1 && F.m2p_item_leaf.size() == F.m2p_item_row.size(), "chains");
    size_t item = 0, chains = 0;
    for (int l = 0; l < nl && (int)F.m2p_chain_ptr.size() == nl + 1; ++l) {
      std::vector<int> path;                           // leaf first
      for (int b = hp.leaf_box[l];; b = hp.box_parent[b]) { if (hp.m2l_ptr[b + 1] > hp.m2l_ptr[b]) path.push_back(b); if (b == 0) break; }
      const int a = F.m2p_chain_ptr[l], e = F.m2p_chain_ptr[l + 1];
      CHECK(e - a == (int)path.size(), "leaf %d: chain of %d boxes, path holds %zu", l, e - a, path.size());
      for (int k = a; k < e && e - a == (int)path.size(); ++k) {
        CHECK(F.m2p_chain_box[k] == path[path.size() - 1 - (k - a)], "leaf %d chain entry %d", l, k - a);
        if (k > a) CHECK(hp.box_level[F.m2p_chain_box[k]] > hp.box_level[F.m2p_chain_box[k - 1]], "leaf %d: chain not root first", l);
      }
      chains += !path.empty();
      for (int r = 0; r < rows_of(hp, l) && !path.empty(); r += 64, ++item)
        CHECK(item < F.m2p_item_leaf.size() && F.m2p_item_leaf[item] == l && F.m2p_item_row[item] == r, "leaf %d: item of row %d", l, r);
    }
    CHECK(item == F.m2p_item_leaf.size(), "M2P items");
    std::printf("m2p chains %zu items %zu\n", chains, item);
  } else CHECK(F.m2p_chain_ptr.empty() && F.m2p_chain_box.empty() && F.m2p_item_leaf.empty(), "M2P work on a plan that is no treecode");

  std::printf("summary f32 %d sym %d items %zu sym_items %zu rc_items %zu owned %d-%d failures %d\n", (int)L.f32, (int)L.stokes_sym, L.items.size(),
              L.sym_items.size(), L.rc_items.size(), hp.leaf_begin, hp.leaf_end, g_fail);
  return g_fail ? 1 : 0;
}
