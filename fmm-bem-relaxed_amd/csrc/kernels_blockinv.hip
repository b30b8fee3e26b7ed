// kernels_blockinv.hip -- the exact block-Jacobi preconditioner of a BLOCK_DIAGONAL plan (blockinv.hpp; include/fmmbem.h
// fmmbem_plan_block_inverse_*).  The plan holds every leaf's self block assembled in HBM (EvalDiagonalSparse,
// examples/BEM/BlockDiagonalPC.hpp:16-60 runs an inner GMRES on it); here the blocks are inverted once and the
// preconditioner becomes one streaming pass per Krylov iteration:
//   blockinv_build_kernel   one workgroup per leaf: the block is read into the inverse's own storage (column-major) and
//                           inverted in place, in global memory, by Gauss-Jordan elimination with partial pivoting
//   blockinv_apply_kernel   z = M v for up to kBlockInvVecs vectors per pass: lane = row, loop over the columns
// Every sum and every pivot choice is fixed by the inputs: the same bits on every run, for every k and every grid.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "blockinv.hpp"

namespace fmmbem {
namespace {

constexpr int kInvThreads = 256;
constexpr int kInvWaves = kInvThreads / 64;

// the better of two pivot candidates: the larger magnitude, the lower row among equals (a NaN never wins)
__device__ __forceinline__ void pivot_pick(double& mag, double& val, int& row, double omag, double oval, int orow) {
  if (omag > mag || (omag == mag && orow < row)) { mag = omag; val = oval; row = orow; }
}

// One workgroup per owned leaf.  W = the leaf's m x m block, entry (i, j) at W[j * m + i].  Step k of the elimination:
//   1. pivot = the largest |W(i, k)|, i >= k, the lowest such row; rows k and pivot change places
//   2. row k: W(k, k) = 1, then the row is divided by the pivot
//   3. every other row i: f = W(i, k); W(i, k) = 0; W(i, :) -= f W(k, :)
// which leaves (P A)^-1 = A^-1 P^-1 in W; the row exchanges are undone on the columns, last first.  The 3 m^2 passes over
// the block are coalesced (consecutive lanes, consecutive rows of one column) and served from the L2.
__global__ __launch_bounds__(kInvThreads) void blockinv_build_kernel(DevicePlan d, BlockInvDev b, const int* __restrict__ selfcol) {
  __shared__ double srow[kBlockInvMax], scol[kBlockInvMax];
  __shared__ int spiv[kBlockInvMax];
  __shared__ double wmag[kInvWaves], wval[kInvWaves];
  __shared__ int wrow[kInvWaves];
  const int t = d.leaf_begin + (int)blockIdx.x;
  const int dof = d.dof, m = dof * d.leaf_nrows[t];
  if (m > kBlockInvMax) return;                          // the host refuses such a plan before it launches
  double* W = b.val + b.off[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sc = selfcol[t];

  if (d.near_sym) {                                     // Stokes, six values per panel pair: (xx,xy) (xz,yy) (yz,zz), three planes per panel row
    const int ncp = d.near_ncols[t];
    const double* sym = d.near_sym + d.near_sym_off[t];
    for (int i = wave; i < m; i += kInvWaves) {
      const int tr = i / 3, a = i - 3 * tr;
      const double* row = sym + (int64_t)tr * 6 * ncp;
      for (int j = lane; j < m; j += 64) {
        const int cp = j / 3, c = j - 3 * cp;
        const int lo = a < c ? a : c, hi = a < c ? c : a;
        const int s = lo == 0 ? hi : lo == 1 ? 2 + hi : 5;          // index in xx xy xz yy yz zz
        W[(int64_t)j * m + i] = row[2 * ((int64_t)(s >> 1) * ncp + sc / 3 + cp) + (s & 1)];
      }
    }
  } else {                                              // rows of near_val: Laplace, or Stokes with nine values per pair
    const double* blk = d.near_val + d.near_off[t];
    const int stride = d.near_stride[t];
    for (int i = wave; i < m; i += kInvWaves)
      for (int j = lane; j < m; j += 64) W[(int64_t)j * m + i] = blk[(int64_t)i * stride + sc + j];
  }
  __syncthreads();

  for (int k = 0; k < m; ++k) {
    double* colk = W + (int64_t)k * m;
    double mag = -1.0, val = 0.0;
    int row = INT_MAX;
    for (int i = k + tid; i < m; i += kInvThreads) {
      const double v = colk[i];
      if (fabs(v) > mag) { mag = fabs(v); val = v; row = i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double om = __shfl_xor(mag, o, 64), ov = __shfl_xor(val, o, 64);
      const int orow = __shfl_xor(row, o, 64);
      pivot_pick(mag, val, row, om, ov, orow);
    }
    if (lane == 0) { wmag[wave] = mag; wval[wave] = val; wrow[wave] = row; }
    __syncthreads();
    mag = wmag[0]; val = wval[0]; row = wrow[0];
#pragma unroll
    for (int w = 1; w < kInvWaves; ++w) pivot_pick(mag, val, row, wmag[w], wval[w], wrow[w]);
    if (!(mag > 0.0) || isinf(mag)) {                   // the same for every thread: a zero or non-finite pivot ends this leaf
      if (tid == 0) atomicMin(b.bad, t);
      return;
    }
    const int p = row;
    const double pv = val;
    if (tid == 0) spiv[k] = p;
    for (int j = tid; j < m; j += kInvThreads) {        // exchange rows k and p, scale the new row k
      double* cj = W + (int64_t)j * m;
      const double a = cj[k], c = cj[p];
      if (p != k) cj[p] = a;
      const double r = (j == k ? 1.0 : c) / pv;
      cj[k] = r;
      srow[j] = r;
    }
    __syncthreads();
    for (int i = tid; i < m; i += kInvThreads) scol[i] = i == k ? 0.0 : colk[i];
    __syncthreads();
    for (int j = wave; j < m; j += kInvWaves) {
      double* cj = W + (int64_t)j * m;
      const double rj = srow[j];
      for (int i = lane; i < m; i += 64) {
        if (i == k) continue;
        const double w0 = j == k ? 0.0 : cj[i];
        cj[i] = fma(-scol[i], rj, w0);
      }
    }
    __syncthreads();
  }
  for (int k = m - 1; k >= 0; --k) {
    const int p = spiv[k];
    if (p == k) continue;
    double *ck = W + (int64_t)k * m, *cp = W + (int64_t)p * m;
    for (int i = tid; i < m; i += kInvThreads) { const double a = ck[i]; ck[i] = cp[i]; cp[i] = a; }
    __syncthreads();
  }
}

// One workgroup per owned leaf, KB vectors per pass.  The leaf's slices of the vectors are gathered through the plan's
// permutation into LDS ([column][vector]: a lane reads the KB values of a column as one broadcast); thread r keeps row r's
// KB sums, acc = fma(M(r, c), v_c, acc) for c = 0, 1, ... -- column c of the inverse is m consecutive doubles, so a
// wavefront's load is one 512-byte run and no sum crosses lanes -- and scatters them back through the permutation.
template <int KB>
__global__ __launch_bounds__(256) void blockinv_apply_kernel(DevicePlan d, BlockInvDev b, const double* __restrict__ v, size_t ldv,
                                                              double* __restrict__ z, size_t ldz) {
  extern __shared__ double sv[];                        // [m][KB]
  const int t = d.leaf_begin + (int)blockIdx.x;
  const int dof = d.dof, m = dof * d.leaf_nrows[t], row0 = d.leaf_row0[t];
  const double* __restrict__ inv = b.val + b.off[blockIdx.x];
  for (int u = threadIdx.x; u < m; u += blockDim.x) {
    const int pr = u / dof;
    const size_t at = (size_t)d.perm[row0 + pr] * dof + (u - pr * dof);
#pragma unroll
    for (int j = 0; j < KB; ++j) sv[u * KB + j] = v[j * ldv + at];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < m; r += blockDim.x) {
    double acc[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) acc[j] = 0.0;
    const double* __restrict__ col = inv + r;
#pragma unroll 8
    for (int c = 0; c < m; ++c) {
      const double a = col[(int64_t)c * m];
#pragma unroll
      for (int j = 0; j < KB; ++j) acc[j] = fma(a, sv[c * KB + j], acc[j]);
    }
    const int pr = r / dof;
    const size_t at = (size_t)d.perm[row0 + pr] * dof + (r - pr * dof);
#pragma unroll
    for (int j = 0; j < KB; ++j) z[j * ldz + at] = acc[j];
  }
}

}  // namespace

hipError_t launch_blockinv_build(const DevicePlan& d, const BlockInvDev& b, const int* selfcol, hipStream_t s) {
  const int nb = d.leaf_end - d.leaf_begin;
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(blockinv_build_kernel, dim3(nb), dim3(kInvThreads), 0, s, d, b, selfcol);
  return hipGetLastError();
}

hipError_t launch_blockinv_apply(const DevicePlan& d, const BlockInvDev& b, int max_m, int k, const double* v, size_t ldv, double* z,
                                 size_t ldz, hipStream_t s) {
  const int nb = d.leaf_end - d.leaf_begin;
  if (nb <= 0 || k <= 0) return hipSuccess;
  if (max_m < 1 || max_m > kBlockInvMax) return hipErrorInvalidValue;
  const int threads = max_m >= 256 ? 256 : (max_m + 63) & ~63;      // a wavefront per leaf where the leaves are small
  for (int j0 = 0; j0 < k; j0 += kBlockInvVecs) {
    const int kb = k - j0 < kBlockInvVecs ? k - j0 : kBlockInvVecs;
    const double* vj = v + (size_t)j0 * ldv;
    double* zj = z + (size_t)j0 * ldz;
    const size_t lds = sizeof(double) * (size_t)max_m * kb;
    switch (kb) {
      case 1: hipLaunchKernelGGL(blockinv_apply_kernel<1>, dim3(nb), dim3(threads), lds, s, d, b, vj, ldv, zj, ldz); break;
      case 2: hipLaunchKernelGGL(blockinv_apply_kernel<2>, dim3(nb), dim3(threads), lds, s, d, b, vj, ldv, zj, ldz); break;
      case 3: hipLaunchKernelGGL(blockinv_apply_kernel<3>, dim3(nb), dim3(threads), lds, s, d, b, vj, ldv, zj, ldz); break;
      default: hipLaunchKernelGGL(blockinv_apply_kernel<4>, dim3(nb), dim3(threads), lds, s, d, b, vj, ldv, zj, ldz); break;
    }
  }
  return hipGetLastError();
}

}  // namespace fmmbem
