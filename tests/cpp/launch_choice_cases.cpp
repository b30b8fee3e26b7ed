// launch_choice_cases.cpp -- host-only program of tests/test_launch_choice_host.py: fills DevicePlan fields by hand and prints what
// csrc/launch_choice.hpp chooses, one line per case.  Built with plain g++ (no device code, no HIP runtime linked).
#include <cstdio>

#include "../../fmm-bem-relaxed_amd/csrc/launch_choice.hpp"

using namespace fmmbem;

static const char* name(NearForm f) {
  switch (f) {
    case NearForm::Hybrid: return "Hybrid";
    case NearForm::Empty: return "Empty";
    case NearForm::Sym3: return "Sym3";
    case NearForm::Pipe: return "Pipe";
    default: return "Plain";
  }
}
static const char* name(P2MForm f) {
  switch (f) {
    case P2MForm::Empty: return "Empty";
    case P2MForm::Invalid: return "Invalid";
    case P2MForm::Recurrence: return "Recurrence";
    case P2MForm::Apply: return "Apply";
    default: return "Stream";
  }
}

static const char* name(ShiftForm f) { return f == ShiftForm::Lanes ? "Lanes" : f == ShiftForm::Rot ? "Rot" : "Sparse"; }

static double sym_vals[2];
static uint8_t rec_flags[1];
static double2 tab_recs[1];
static int4 item_recs[1];

// a Laplace plan with a stored near matrix and stored P2M moments
static DevicePlan laplace() {
  DevicePlan d;
  d.dof = 1; d.max_runs = 10; d.near_nitems = 5000;
  d.near_rec = nullptr; d.near_sym = nullptr; d.sym_items = nullptr; d.sym_nitems = 0;
  d.n_p2m = 1000; d.p2m_tab = tab_recs; d.n_act = 1;
  return d;
}
static DevicePlan stokes() {
  DevicePlan d = laplace();
  d.dof = 3; d.near_sym = sym_vals; d.sym_items = item_recs; d.sym_nitems = 3000; d.n_act = 4;
  return d;
}

static void near(const char* what, const DevicePlan& d) {
  const NearForm f = near_form(d);
  if (f == NearForm::Hybrid || f == NearForm::Empty) std::printf("near %s %s\n", what, name(f));
  else std::printf("near %s %s grid=%d lds=%zu\n", what, name(f), near_grid(d, f), near_lds(d, f));
}
static void p2m(const char* what, const DevicePlan& d, int p) {
  const P2MForm f = p2m_form(d, p);
  if (f == P2MForm::Empty || f == P2MForm::Invalid) std::printf("p2m %s %s\n", what, name(f));
  else std::printf("p2m %s %s grid=%d\n", what, name(f), p2m_grid(d, f));
}

// the tree-pass rule: the switches of a geometry and what the kernels' translation units answer for the order, all at their defaults
struct ShiftSwitches { bool rot = true, lanes = true; int lanes_max = -1, rot_min = 2048; bool lanes_ok = true, rot_ok = true; };
static void shift(const char* set, const ShiftSwitches& c, bool m2m, int p, int pairs, int n_act, int level_boxes = 0) {
  std::printf("shift %s_%s_p%d_%dx%d_boxes%d %s\n", set, m2m ? "M2M" : "L2L", p, pairs, n_act, level_boxes,
              name(shift_form(c.rot, c.lanes, c.lanes_max, c.rot_min, pairs, level_boxes, p, n_act, m2m, c.lanes_ok, c.rot_ok)));
}
// the hand-over from the wavefront kernel to the rotation kernel, per pass and order, in pair-slots
static void shift_thresholds(const char* set, const ShiftSwitches& c) {
  for (int d : {0, 1}) {
    shift(set, c, true, 8, 2048 + d, 1); shift(set, c, true, 8, 512 + d, 4);
    shift(set, c, true, 9, 8192 + d, 1); shift(set, c, true, 10, 16384 + d, 1); shift(set, c, true, 11, 2048 + d, 1);
    shift(set, c, false, 3, 16384 + d, 1); shift(set, c, false, 10, 4096 + d, 4);
  }
}

int main() {
  DevicePlan d = laplace();
  d.max_runs = 256; near("runs256", d);
  d.max_runs = 257; near("runs257", d);
  d = stokes(); near("stokes_sym", d);
  d.near_sym = nullptr; near("stokes_full", d);
  d = laplace(); d.near_rec = rec_flags; near("hybrid", d);
  d.near_nitems = 0; near("hybrid_empty", d);
  d = laplace(); d.near_nitems = 0; near("empty", d);
  for (int n : {1279, 1280, 1281}) { d = laplace(); d.near_nitems = n; char w[32]; std::snprintf(w, sizeof w, "items%d", n); near(w, d); }

  d = laplace();
  p2m("p7", d, 7); p2m("p8", d, 8); p2m("p0", d, 0); p2m("p16", d, 16); p2m("p17", d, 17);
  d.n_act = 2; p2m("two_slots", d, 8);
  d = laplace(); d.p2m_tab = nullptr; p2m("no_table", d, 8);
  d = laplace(); d.n_p2m = 0; p2m("no_leaves", d, 8); p2m("no_leaves_p0", d, 0);
  for (int n : {8188, 8192, 8196}) { d = laplace(); d.n_p2m = n; char w[32]; std::snprintf(w, sizeof w, "leaves%d", n); p2m(w, d, 8); }
  d = laplace(); d.n_p2m = 20000; p2m("apply_cap", d, 7);
  d.p2m_tab = nullptr; p2m("recurrence_cap", d, 7);

  // the combined launch: every pairing of a near form with a P2M form
  for (int nf = 0; nf < 5; ++nf)
    for (int pf = 0; pf < 5; ++pf) {
      d = laplace();
      if (nf == 0) d.near_rec = rec_flags;
      if (nf == 1) d.near_nitems = 0;
      if (nf == 2) d = stokes(), d.n_act = 1;
      if (nf == 4) d.max_runs = 300;
      int p = 8;
      if (pf == 0) d.n_p2m = 0;
      if (pf == 1) p = 17;
      if (pf == 2) d.p2m_tab = nullptr;
      if (pf == 3) p = 7;
      std::printf("fused %s+%s %d\n", name(near_form(d)), name(p2m_form(d, p)), (int)near_p2m_ok(d, p));
    }

  // multi-vector passes
  d = laplace();
  for (int nv : {2, 4, 8}) std::printf("multi Pipe nv=%d grid=%d lds=%zu\n", nv, near_grid(d, NearForm::Pipe, nv), near_lds(d, NearForm::Pipe, nv));
  d = stokes();
  for (int nv : {2, 3, 4}) std::printf("multi Sym3 nv=%d grid=%d lds=%zu\n", nv, near_grid(d, NearForm::Sym3, nv), near_lds(d, NearForm::Sym3, nv));
  std::printf("batch_near_ok laplace=%d runs257=%d stokes=%d hybrid=%d\n", (int)batch_near_ok(laplace()),
              (int)batch_near_ok([] { DevicePlan e = laplace(); e.max_runs = 257; return e; }()), (int)batch_near_ok(stokes()),
              (int)batch_near_ok([] { DevicePlan e = laplace(); e.near_rec = rec_flags; return e; }()));
  for (int w : {1, 2, 4, 5}) std::printf("sym3_ok width=%d %d\n", w, (int)batch_near_sym3_ok(d, w));
  d.max_runs = 7680; std::printf("sym3_ok runs7680 %d\n", (int)batch_near_sym3_ok(d, 4));
  d.max_runs = 7681; std::printf("sym3_ok runs7681 %d\n", (int)batch_near_sym3_ok(d, 4));
  std::printf("sym3_ok laplace %d\n", (int)batch_near_sym3_ok(laplace(), 2));
  d = stokes(); d.sym_items = nullptr; std::printf("sym3_ok no_items %d\n", (int)batch_near_sym3_ok(d, 2));
  std::printf("near_f32_ok %d%d%d%d\n", (int)near_f32_ok(1, 256, false), (int)near_f32_ok(1, 257, false), (int)near_f32_ok(3, 999, true), (int)near_f32_ok(3, 10, false));

  ShiftSwitches c;
  shift_thresholds("dflt", c);
  for (bool m2m : {true, false}) shift("dflt", c, m2m, 10, 1 << 30, 4);     // 2^32 pair-slots: a 64-bit product, not 0
  shift("dflt", c, true, 10, 1, 1, 0);
  c = ShiftSwitches{}; c.lanes = false;
  shift("lanes_off", c, true, 10, 1, 1, 2047); shift("lanes_off", c, true, 10, 1, 1, 2048);
  c = ShiftSwitches{}; c.lanes_ok = false;
  shift("lanes_unsupported", c, true, 10, 1, 1, 0);
  c = ShiftSwitches{}; c.rot = false;
  shift_thresholds("rot_off", c);
  shift("rot_off", c, true, 10, 1, 1, 2048);
  c = ShiftSwitches{}; c.lanes_ok = c.rot_ok = false;                       // p > 12
  shift_thresholds("unsupported", c);
  shift("unsupported", c, true, 10, 1, 1, 2048);
  c = ShiftSwitches{}; c.lanes_max = 100;
  for (int n : {100, 101}) { shift("max100", c, true, 10, n, 1); shift("max100", c, false, 3, n, 1); }
  return 0;
}
