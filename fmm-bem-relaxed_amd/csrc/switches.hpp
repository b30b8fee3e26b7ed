// switches.hpp -- every environment switch of the library, each read in ONE place (INTEGRATION.md lists the same names;
// tests/test_switches_doc.py holds the two together).  Host code only.  When a switch is read is part of its contract:
//   live     at every launch / execute / call: tests flip these inside one process
//   plan     while a plan (or its geometry) is created
//   process  once, at the first use in the process
// A switch whose default differs between call sites reports "unset" (an empty optional) and the call site keeps its default.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <optional>
#include <vector>

namespace fmmbem {
namespace sw {

// ---- the three ways a switch is parsed ----
inline bool flag(const char* name, bool dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) != 0 : dflt; }
inline std::optional<int> integer(const char* name) { const char* e = std::getenv(name); return e ? std::optional<int>(std::atoi(e)) : std::nullopt; }
inline bool present(const char* name) { return std::getenv(name) != nullptr; }

// ---- live ----
inline int near_p2m() { return integer("FMMBEM_NEAR_P2M").value_or(1); }             // 0: two launches, 1: one where eligible, 2: one or an error
inline bool p2m_stream() { return flag("FMMBEM_P2M_STREAM", true); }
inline bool l2p_scatter() { return flag("FMMBEM_L2P_SCATTER", true); }
inline bool l2p_generic() { return flag("FMMBEM_L2P_GENERIC", false); }
inline bool ops_generic() { return flag("FMMBEM_OPS_GENERIC", false); }
inline bool multi_issue_threads() { return flag("FMMBEM_MULTI_ISSUE_THREADS", true); }

// ---- plan ----
inline bool build_trace() { return present("FMMBEM_BUILD_TRACE"); }              // on when set to anything
inline bool graph(bool dflt) { return flag("FMMBEM_GRAPH", dflt); }              // default off; on for the shards of a device list
inline double near_stream_fraction(double dflt) { const char* e = std::getenv("FMMBEM_NEAR_STREAM_FRACTION"); return e ? std::atof(e) : dflt; }
inline bool stokes_sym() { return flag("FMMBEM_STOKES_SYM", true); }
inline bool m2l_rot() { return flag("FMMBEM_M2L_ROT", true); }
inline bool shift_lanes(bool dflt) { return flag("FMMBEM_SHIFT_LANES", dflt); }
inline int shift_lanes_max(int dflt) { return integer("FMMBEM_SHIFT_LANES_MAX").value_or(dflt); }
inline bool shift_rot(bool dflt) { return flag("FMMBEM_SHIFT_ROT", dflt); }
inline int shift_rot_min(int dflt) { return integer("FMMBEM_SHIFT_ROT_MIN").value_or(dflt); }
inline bool p2m_table() { return flag("FMMBEM_P2M_TABLE", true); }
inline bool p2m_table_points() { return flag("FMMBEM_P2M_TABLE_POINTS", true); }
inline bool asm_cols() { return flag("FMMBEM_ASM_COLS", true); }
inline bool multi_upward(bool dflt) { return flag("FMMBEM_MULTI_UPWARD", dflt); }
inline bool plan_share() { return flag("FMMBEM_PLAN_SHARE", true); }
inline bool panels_on_host() { return flag("FMMBEM_PANELS_ON_HOST", false); }
inline bool build_two_phase() { return flag("FMMBEM_BUILD_TWO_PHASE", true); }
inline bool tree_serial() { return flag("FMMBEM_TREE_SERIAL", false); }
inline int rot_long_rounds() { return std::max(0, integer("FMMBEM_ROT_LONG_ROUNDS").value_or(0)); }     // 0: by the rule of its call site
inline int rot_item_passes() { return std::max(1, integer("FMMBEM_ROT_ITEM_PASSES").value_or(2)); }
inline int rot_long_max() { return std::max(1, integer("FMMBEM_ROT_LONG_MAX").value_or(16)); }
inline std::vector<int> devices() {                                              // "0,1,...": fewer than two ordinals count as unset
  std::vector<int> out;
  if (const char* e = std::getenv("FMMBEM_DEVICES"))
    for (const char* c = e; *c;) { char* end = nullptr; const long v = std::strtol(c, &end, 10); if (end == c) break; out.push_back((int)v); c = *end ? end + 1 : end; }
  if (out.size() < 2) out.clear();
  return out;
}

// ---- process ----
inline std::optional<int> hyb_wg_stream() { static const std::optional<int> v = integer("FMMBEM_HYB_WG_STREAM"); return v; }          // defaults 2 (Stokes), 3 (Laplace)
inline std::optional<int> hyb_wg_recompute() { static const std::optional<int> v = integer("FMMBEM_HYB_WG_RECOMPUTE"); return v; }    // defaults 1, 2 (Stokes, sources in LDS)
inline std::optional<int> f32_shape() { static const std::optional<int> v = integer("FMMBEM_F32_SHAPE"); return v; }                  // defaults 0 (Stokes), 1 (Laplace)
inline int batch_shape() { static const int v = integer("FMMBEM_BATCH_SHAPE").value_or(0); return v; }
inline int batch_nv() { static const int v = integer("FMMBEM_BATCH_NV").value_or(4); return v == 2 || v == 8 ? v : 4; }
inline int krylov_fail_grow() { static const int v = integer("FMMBEM_KRYLOV_FAIL_GROW").value_or(0); return v; }

}  // namespace sw
}  // namespace fmmbem
