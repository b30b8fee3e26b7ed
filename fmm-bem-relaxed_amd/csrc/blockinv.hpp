// blockinv.hpp -- the exact block-Jacobi preconditioner of a BLOCK_DIAGONAL plan (include/fmmbem.h,
// fmmbem_plan_block_inverse_*): what the kernels of kernels_blockinv.hip take by value, and their launchers.
// Kept apart from device_launch.hpp so that it rebuilds nothing but its two users.
#pragma once
#include "device_plan.hpp"

namespace fmmbem {

// The largest leaf block the kernels serve, in unknowns (ncrit * dof): the apply kernel stages kBlockInvVecs slices of v in
// LDS (4 x 768 x 8 B = 24 KiB), the inversion kernel one row and one column (12 KiB).  Defaults are 64 (Laplace), 192 (Stokes).
constexpr int kBlockInvMax = 768;
constexpr int kBlockInvVecs = 4;                      // vectors one pass over the inverses serves

// Storage the inverse owns: per owned leaf t (index t - leaf_begin) the inverse of its self block, m x m with
// m = dof * leaf_nrows[t], COLUMN-major without padding at val + off[t - leaf_begin]: entry (row r, column c) at c * m + r,
// so that the lanes of a wavefront (lane = row) read consecutive addresses for every column.
struct BlockInvDev {
  double* val = nullptr;
  const int64_t* off = nullptr;                       // [owned leaves + 1]
  int* bad = nullptr;                                 // lowest leaf whose elimination met a zero or non-finite pivot (INT_MAX: none)
};

// Reads every owned leaf's self block from the plan's assembled matrix (selfcol[leaf]: first column, in unknowns, of the
// leaf's own panels in its row block) and inverts it in place in b.val by Gauss-Jordan with partial pivoting.
hipError_t launch_blockinv_build(const DevicePlan& d, const BlockInvDev& b, const int* selfcol, hipStream_t s);
// z_j = M v_j, j < k; vector j at v + j * ldv, result at z + j * ldz; both in the caller's panel order.  threads: 64..256.
hipError_t launch_blockinv_apply(const DevicePlan& d, const BlockInvDev& b, int max_m, int k, const double* v, size_t ldv, double* z,
                                 size_t ldz, hipStream_t s);

}  // namespace fmmbem
