// plan_layout_cases.cpp -- host-only program of tests/test_plan_layout_host.py: calls the cutters of csrc/plan_layout.hpp on inputs
// written by hand and prints what they return, one line per case.  Built with plain g++ (no device code, no HIP runtime linked).
#include <cstdio>
#include <vector>

#include "../../fmm-bem-relaxed_amd/csrc/plan_layout.hpp"

using namespace fmmbem;

static void rows(const char* what, int n, int64_t row_bytes, int64_t item_bytes) {
  std::vector<WorkItem> out;
  cut_rows(7, n, row_bytes, item_bytes, out);
  std::printf("rows %s", what);
  for (const WorkItem& w : out) {
    std::printf(" %d+%d", w.r0, w.nr);
    if (w.leaf != 7 || w.key != w.nr * row_bytes) std::printf("!");
  }
  std::printf("\n");
}
static void recompute(const char* what, int n, int ncp, int cap) {
  std::vector<WorkItem> out;
  cut_recompute(7, n, ncp, cap, out);
  std::printf("recompute %s", what);
  for (const WorkItem& w : out) {
    std::printf(" %d+%d", w.r0, w.nr);
    if (w.leaf != 7 || w.key != (int64_t)w.nr * ncp) std::printf("!");
  }
  std::printf("\n");
}
static void ints(const char* kind, const char* what, const std::vector<int>& v) {
  std::printf("%s %s", kind, what);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
static void single_pass(const char* what, const std::vector<int>& seg_len, int base) {
  std::vector<int> ptr;
  cut_single_pass(seg_len, base, ptr);
  ints("pass", what, ptr);
}
static void side(const char* what, const std::vector<int>& counts, int64_t row_begin, int64_t row_end) {
  std::vector<int64_t> ptr(counts.size() + 1, 0);
  for (size_t i = 0; i < counts.size(); ++i) ptr[i + 1] = ptr[i] + counts[i];
  std::printf("side %s", what);
  for (const int4& it : cut_side_items(counts, ptr, row_begin, row_end)) std::printf(" %d:%d,%d:%d", it.x, it.y, it.z, it.w);
  std::printf("\n");
}

int main() {
  const int64_t K256 = 256 << 10, K512 = 512 << 10;
  if (kNearItemBytes != K256 || kSymItemBytes != K512) { std::printf("item sizes changed\n"); return 1; }
  rows("r1", 1, 1024, K256); rows("r3", 3, 1024, K256); rows("r4", 4, 1024, K256);
  rows("r7", 7, 1024, K256); rows("r8", 8, 1024, K256); rows("r9", 9, 1024, K256);
  rows("fits", 64, 4096, K256); rows("one_over", 65, 4096, K256); rows("redeal", 100, 4096, K256);
  rows("wide10", 10, 300000, K256); rows("wide3", 3, 300000, K256); rows("wide1", 1, 300000, K256);
  rows("coarse58", 58, 128248, K256);
  rows("sym512", 20, 48 * 1000, K512); rows("sym256", 20, 48 * 1000, K256); rows("sym512_fits", 64, 48 * 170, K512);
  recompute("cap32_r32", 32, 10, 32); recompute("cap32_r33", 33, 10, 32); recompute("cap32_r61", 61, 10, 32);
  recompute("cap60_r60", 60, 10, 60); recompute("cap60_r61", 61, 10, 60); recompute("cap60_r1", 1, 10, 60);
  ints("l2p", "rows64", l2p_groups({32, 32}, 8)); ints("l2p", "rows65", l2p_groups({32, 33}, 8));
  ints("l2p", "nine_max8", l2p_groups(std::vector<int>(9, 1), 8)); ints("l2p", "nine_max4", l2p_groups(std::vector<int>(9, 1), 4));
  ints("l2p", "big_between", l2p_groups({10, 100, 10}, 8)); ints("l2p", "big_first", l2p_groups({100, 5}, 8));
  ints("l2p", "empty", l2p_groups({}, 8));
  single_pass("pairs64", std::vector<int>(8, 8), 0);
  { std::vector<int> v(8, 8); v.push_back(1); single_pass("pairs65", v, 0); single_pass("pairs65_base100", v, 100); }
  single_pass("none", {}, 5);
  side("e256", {128, 128}, 0, 2); side("e257", {128, 129}, 0, 2); side("row300", {5, 300, 5}, 0, 3);
  side("empty_row", {3, 0, 4}, 0, 3); side("rows300", std::vector<int>(300, 1), 0, 300); side("owned_1_3", {1, 1, 1, 1}, 1, 3);
  side("nothing", {0, 0}, 0, 2);
  return 0;
}
