// launch_choice.hpp -- which kernel a launch takes, on which grid, with how much dynamic LDS: every rule written ONCE, as a plain
// function of the DevicePlan (and the order p, and the vectors of a batched pass).  The launchers of kernels_near.hip and
// kernels_far.hip, the predicates a plan asks before it chooses a path, and the launch that runs two kernels as one grid all call
// these: the alternative paths give the same bits because they agree on them.  Host code only.
#pragma once
#include "device_plan.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace fmmbem {

constexpr int kWave = 64;

// ---------------------------------------- near field (kernels_near.hip) ----------------------------------------
constexpr int kSpmvWaves = 4;
constexpr int kSpmvChunk = 2048;                      // plain form: columns of x staged in LDS at a time (16 KiB)
constexpr int kSpmvPipeChunk = 1024;                  // pipelined form: columns per x buffer (2 x 8 KiB)
constexpr int kSpmvOcc = 5;                           // wavefronts per SIMD = workgroups per CU (82 VGPRs)
#ifndef FMMBEM_SYM_OCC
#define FMMBEM_SYM_OCC 5
#endif
#ifndef FMMBEM_SYM_CHUNK
#define FMMBEM_SYM_CHUNK 1024
#endif
constexpr int kSymOcc = FMMBEM_SYM_OCC;               // sym3: workgroups per CU
constexpr int kSymChunk = FMMBEM_SYM_CHUNK;           // sym3: source panels of x staged at a time (3 x 8 KiB)
constexpr int batch_occ(int nv) { return nv <= 2 ? 4 : nv <= 4 ? 2 : 1; }              // workgroups per CU, pipelined form, 2 / 4 / 8 vectors
constexpr int sym3_multi_occ(int nv) { return nv <= 2 ? 3 : nv == 3 ? 2 : 1; }         // ... that 24 KiB of x per vector leave sym3
constexpr size_t kSym3MultiLds = 156 * 1024;          // most dynamic LDS of a multi-vector sym3 pass, within the 160 KiB of a CU

// Hybrid: near_rec is set (launch_near_hybrid; launch_near_spmv refuses it).  Sym3: Stokes with the symmetric blocks.  Pipe: one
// unknown per panel, the pipelined kernel, which prefetches an item's run descriptors one per thread; a leaf with more runs than
// threads (never seen) takes Plain, as does Stokes with the full 3 x 3 rows.
enum class NearForm { Hybrid, Empty, Sym3, Pipe, Plain };
inline bool near_pipe_ok(int dof, int max_runs) { return dof == 1 && max_runs <= kSpmvWaves * kWave; }
inline NearForm near_kernel(const DevicePlan& d) {    // the form of the plan's items, whether or not there are any
  if (d.near_rec) return NearForm::Hybrid;
  if (d.dof == 3 && d.near_sym) return NearForm::Sym3;
  return near_pipe_ok(d.dof, d.max_runs) ? NearForm::Pipe : NearForm::Plain;
}
inline NearForm near_form(const DevicePlan& d) {
  const NearForm k = near_kernel(d);
  return k != NearForm::Hybrid && d.near_nitems <= 0 ? NearForm::Empty : k;
}
// The grid is exactly what is resident at once (workgroups per CU x 256 CUs): with one more per CU the stragglers start when the
// others finish (0.98 ms instead of 0.79 at N = 1M).  nv: 1, or a count the multi-vector kernel is instantiated for.
inline int near_occ(NearForm f, int nv) { return f == NearForm::Sym3 ? (nv == 1 ? kSymOcc : sym3_multi_occ(nv)) : nv == 1 ? kSpmvOcc : batch_occ(nv); }
inline int near_grid(const DevicePlan& d, NearForm f, int nv = 1) { return std::min(f == NearForm::Sym3 ? d.sym_nitems : d.near_nitems, 256 * near_occ(f, nv)); }
inline size_t near_lds(const DevicePlan& d, NearForm f, int nv = 1) {      // the x buffers, then the run descriptors
  const size_t runs = (size_t)d.max_runs * sizeof(int);
  return f == NearForm::Pipe   ? 2 * (size_t)nv * kSpmvPipeChunk * sizeof(double) + 4 * runs
         : f == NearForm::Sym3 ? (size_t)nv * 3 * kSymChunk * sizeof(double) + 2 * runs
                               : (size_t)kSpmvChunk * sizeof(double) + 2 * runs;
}
// the plans the float kernels serve (near_f32_max_p; asked before the DevicePlan exists), those launch_near_spmv_multi serves, and
// those launch_near_sym3_multi serves at a pass of `width` vectors (stokes_batch_width)
inline bool near_f32_ok(int dof, int max_runs, bool stokes_sym) { return dof == 3 ? stokes_sym : near_pipe_ok(dof, max_runs); }
inline bool batch_near_ok(const DevicePlan& d) { return near_kernel(d) == NearForm::Pipe; }
inline bool batch_near_sym3_ok(const DevicePlan& d, int width) {
  return near_kernel(d) == NearForm::Sym3 && d.sym_items && width >= 2 && width <= 4 && near_lds(d, NearForm::Sym3, width) <= kSym3MultiLds;
}

// ---------------------------------------- P2M (kernels_far.hip) ----------------------------------------
constexpr int kPmaxDev = 16;
constexpr int kP2MWaves = 4;                          // recurrence form: independent leaves per workgroup
// Recurrence: no stored moments.  Stream: one expansion per box and more than 32 coefficients (p >= 8); FMMBEM_P2M_STREAM is read
// here, at every call.  Apply: the stored moments otherwise.
enum class P2MForm { Empty, Invalid, Recurrence, Apply, Stream };
inline P2MForm p2m_form(const DevicePlan& d, int p) {
  if (d.n_p2m <= 0) return P2MForm::Empty;
  if (p < 1 || p > kPmaxDev) return P2MForm::Invalid;
  if (!d.p2m_tab) return P2MForm::Recurrence;
  return d.n_act == 1 && p * (p + 1) / 2 > kWave / 2 && sw::p2m_stream() ? P2MForm::Stream : P2MForm::Apply;
}
inline int p2m_grid(const DevicePlan& d, P2MForm f) {
  const int per = f == P2MForm::Recurrence ? kP2MWaves : 4;      // leaves per workgroup
  return std::min((d.n_p2m + per - 1) / per, 256 * (f == P2MForm::Apply ? 16 : 8));
}

// The near field and P2M as one launch (near_p2m_kernel), both non-empty.  The caller (fmmbem_plan::run) rules out what it alone
// knows: hybrid and float near fields, target plans, partial executes, stage timing.
inline bool near_p2m_ok(const DevicePlan& d, int p) { return near_form(d) == NearForm::Pipe && p2m_form(d, p) == P2MForm::Stream; }

// ---------------------------------------- M2P (kernels_far.hip, the treecode's far field) ----------------------------------------
constexpr int kM2PWaves = 4;                          // items (<= 64 rows of one leaf) per workgroup, one per wavefront
constexpr int kM2PBatch = 4;                          // sources whose M is staged per LDS fill
// a wavefront's LDS slice: the batch's sources x active slots x S coefficients (7 KB at p = 10, 17 KB at p = 16 with both slots);
// fewer wavefronts per workgroup where four slices pass 48 KB, as L2P
inline size_t m2p_wave_lds(const DevicePlan& d, int p) { return sizeof(double2) * (size_t)kM2PBatch * d.n_act * (p * (p + 1) / 2); }
inline int m2p_waves(const DevicePlan& d, int p) { return (int)std::clamp<size_t>((48 * 1024) / m2p_wave_lds(d, p), 1, kM2PWaves); }
inline size_t m2p_lds(const DevicePlan& d, int p) {   // the tables of fill_l2p_tables (3 S doubles), then the slices
  return sizeof(double2) * (size_t)((3 * (p * (p + 1) / 2) + 1) / 2) + m2p_waves(d, p) * m2p_wave_lds(d, p);
}
inline int m2p_grid(const DevicePlan& d, int p, int n_items) { return std::min((n_items + m2p_waves(d, p) - 1) / m2p_waves(d, p), 256 * 8); }

// ---------------------------------------- tree passes (kernels_shift.hip, kernels_m2l_rot.hip, kernels_far.hip) ----------------------------------------
// One level of the upward / downward pass, p <= 12: the one-pair-per-WAVEFRONT kernel (kernels_shift.hip) for up to
// shift_lanes_max pairs of this plan, the one-pair-per-LANE rotation kernel (kernels_m2l_rot.hip, ~20 us a pass whatever it holds)
// above -- the two give the same bits, so every plan and every shard chooses by its own share.  p > 12 (and FMMBEM_SHIFT_ROT=0):
// the sparse-operator kernels of kernels_far.hip, which round differently -- there the choice is the same for all shards, and
// beside the wavefront kernel never the sparse operators.
enum class ShiftForm { Lanes, Rot, Sparse };
// one pair per WAVEFRONT (kernels_shift.hip, shift_lanes.hpp): the same bits as the one-pair-per-lane kernels, ~5 us for a
// level of a few thousand pairs where a pass of those takes ~20 whatever it holds; LDS-bound above (N = 1M, p = 10, L2L: 5 800
// pairs 10.6 us against 16-20, 21 000 pairs 26 against 19.5, 39 000 pairs 42 against 23.6).  A launch of up to shift_lanes_max
// pairs takes it -- counted on THIS plan's share of the level: the two kernels give the same bits, so a shard may choose for
// itself (FMMBEM_SHIFT_LANES=0: never; FMMBEM_SHIFT_LANES_MAX).  Pairs are counted per live expansion slot
// (Stokes: four, config 4 at p = 8 with the slots uncounted: M2M 0.09 -> 0.18 ms)
// Thresholds from tools/shift_lanes_sweep.sh (profiles/r04k_shift_lanes_sweep.txt; M2M / L2L ms for one GPU and one rank of eight):
// L2L gains at every order up to 16 384 pair-slots; M2M -- whose wavefronts also walk or share a parent's children -- only at
// p = 9, 10, elsewhere the rotation kernel's pass is short enough and only launches of <= 2 048 pair-slots go over.
inline int lanes_max(int shift_lanes_max, int p, bool m2m) {      // shift_lanes_max >= 0: one threshold for both passes and all orders (sweeps)
  return shift_lanes_max >= 0 ? shift_lanes_max : !m2m ? 16384 : p == 10 ? 16384 : p == 9 ? 8192 : 2048;
}
// pairs: of the launch on this plan; level_boxes: boxes of the child level in the whole tree; lanes_ok, rot_ok: what
// shift_lanes_supported(p), shift_rot_supported(p) answer -- the kernels' translation units say which orders they hold
inline ShiftForm shift_form(bool shift_rot, bool shift_lanes, int shift_lanes_max, int shift_rot_min, int pairs, int level_boxes,
                            int p, int n_act, bool m2m, bool lanes_ok, bool rot_ok) {
  if (shift_rot && shift_lanes && lanes_ok && (int64_t)pairs * n_act <= lanes_max(shift_lanes_max, p, m2m)) return ShiftForm::Lanes;
  if (shift_rot && rot_ok && (shift_lanes || level_boxes >= shift_rot_min)) return ShiftForm::Rot;
  return ShiftForm::Sparse;
}

}  // namespace fmmbem
