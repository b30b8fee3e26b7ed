// p2m_stream.hpp -- the body of the streaming P2M (one expansion per box, more than 32 coefficients), shared by the kernels that
// run it: p2m_stream_kernel (kernels_far.hip) and near_p2m_kernel (kernels_near.hip: the P2M workgroups queued behind the near
// field's in one grid).  One text, so the order of every FMA is the same wherever it runs.  What it does and what it does not
// respond to is recorded at p2m_stream_kernel.
#pragma once
#include "device_plan.hpp"

namespace fmmbem {

constexpr int kP2MStream = 8;                         // table entries (panels) in flight per lane
typedef __attribute__((address_space(4))) int ConstInt;
typedef __attribute__((address_space(4))) double ConstDouble;
template <class T, class U>
__device__ __forceinline__ const T* as_const_space(const U* p) { return reinterpret_cast<const T*>(reinterpret_cast<uintptr_t>(p)); }

// Workgroup wg of nwg (four wavefronts each): wavefront wv takes the leaves 4 wg + wv, + 4 nwg, ...  No barrier, no LDS.
__device__ __forceinline__ void p2m_stream_run(const DevicePlan& d, const int P, const int wg, const int nwg) {
  typedef double tvec2 __attribute__((ext_vector_type(2)));   // native 16-B vector (the nontemporal builtin needs it)
  constexpr int kWave = 64;
  constexpr int U = kP2MStream;
  const int S = P * (P + 1) / 2, SM = d.s_max, TS = d.p2m_stride;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const double2* __restrict__ tab = d.p2m_tab - (size_t)d.p2m_tab_row0 * TS;      // indexed by tree-order panel
  const ConstInt* leaf_of = as_const_space<ConstInt>(d.p2m_leaf);
  const ConstInt* box_of = as_const_space<ConstInt>(d.leaf_box);
  const ConstInt* row0_of = as_const_space<ConstInt>(d.leaf_row0);
  const ConstInt* nrows_of = as_const_space<ConstInt>(d.leaf_nrows);
  const ConstDouble* xt = as_const_space<ConstDouble>(d.xt);
  const int slot = d.act[0], stride = nwg * 4, n = d.n_p2m;
  // what this lane streams (at most two items: 128 >= the 120 + 8 of p = 16): the table slot it loads and where the sums go.
  // Classic records: item = coefficient.  Packed records: the complex (n, m >= 1) in order, then the m = 0 reals two to a slot.
  int tslot[2], st0[2], st1[2];
  {
    const int nb = d.p2m_packed ? P * (P - 1) / 2 : S, items = d.p2m_packed ? nb + (P + 1) / 2 : S;
    for (int it = 0; it < 2; ++it) {
      const int item = lane + it * kWave;
      tslot[it] = -1; st0[it] = 0; st1[it] = -2;
      if (item >= items) continue;
      if (!d.p2m_packed) { tslot[it] = item; st0[it] = item; }
      else if (item < nb) {
        int cn = 1;
        while (cn * (cn + 1) / 2 <= item) ++cn;          // degree of packed position `item`
        tslot[it] = item; st0[it] = item + cn + 1;       // n (n + 1) / 2 + m  =  cpos + n + 1
      } else {
        const int k = item - nb;
        tslot[it] = d.p2m_real_off + k;
        st0[it] = (2 * k) * (2 * k + 1) / 2;
        st1[it] = 2 * k + 1 < P ? (2 * k + 1) * (2 * k + 2) / 2 : -1;
      }
    }
  }
  int li = wg * 4 + wv;
  if (li >= n) return;
  int leaf = leaf_of[li];
  int box = box_of[leaf], row0 = row0_of[leaf], nrows = nrows_of[leaf];
  for (; li < n; li += stride) {
    // the next leaf's record, on its way while this one streams
    const int nl = li + stride < n ? li + stride : li;
    const int nleaf = leaf_of[nl];
    const int nbox = box_of[nleaf], nrow0 = row0_of[nleaf], nnrows = nrows_of[nleaf];
    for (int it = 0; it < 2; ++it) {
      if (tslot[it] < 0) break;
      double2 m = {0, 0};
      for (int r = 0; r < nrows; r += U) {
        tvec2 t[U];
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                    // a leaf's last batch is a short one: the row test is scalar, a branch
          t[u] = tvec2{0, 0}; x[u] = 0.0;                //  around the load (re-reading row r instead costs L2 requests: 24 for 19 rows)
          if (r + u < nrows) {
            const int64_t iu = (int64_t)row0 + r + u;
            t[u] = __builtin_nontemporal_load(reinterpret_cast<const tvec2*>(tab + (size_t)iu * TS + tslot[it]));
            x[u] = xt[iu];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { m.x = fma(x[u], t[u].x, m.x); m.y = fma(x[u], t[u].y, m.y); }   // panel order, as p2m_apply_kernel
      }
      double2* Mb = d.M + ((size_t)box * d.nslots + slot) * SM;
      if (st1[it] == -2) Mb[st0[it]] = m;                // a complex coefficient (classic layout, or packed m >= 1)
      else {                                             // a packed pair of m = 0 moments: two real coefficients
        Mb[st0[it]] = double2{m.x, 0.0};
        if (st1[it] >= 0) Mb[st1[it]] = double2{m.y, 0.0};
      }
    }
    leaf = nleaf; box = nbox; row0 = nrow0; nrows = nnrows;
  }
}

}  // namespace fmmbem
