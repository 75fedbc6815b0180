// The fixed-order column sum of fixed_sum.h on the device: the tree across the lanes of a wavefront and the finish of
// up to FS_FIN_COLS columns by one workgroup.  Only .hip files include this header.
#pragma once
#include "fixed_sum.h"
#include <hip/hip_runtime.h>

#define FS_FIN_THREADS (FS_CHAINS * FS_FIN_COLS)

// The tree of fs_tree64 across the 64 lanes of a wavefront, lane r holding a[r]: lane r takes lane r + h for h = 32 .. 1.  Only the
// lanes below h hold meaningful sums, and those are the ones read; the sum is valid in lane 0.  U independent trees go step by step
// side by side, which hides the latency of the six dependent cross-lane steps.
template <int U>
__device__ __forceinline__ void fs_wave_tree64(double (&a)[U]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int h = FS_ROWS / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = a[u] + __shfl_down(a[u], h, FS_ROWS);
  }
}
__device__ __forceinline__ double fs_wave_tree64(double a) {
  double v[1] = {a};
  fs_wave_tree64(v);
  return v[0];
}

// fs_finish for the columns [j0, j0 + FS_FIN_COLS) of part (P, nq): thread q * FS_FIN_COLS + cc is chain q of column j0 + cc, adds the
// partials q, q + 64, .. in ascending order from +0.0 (a column past nq: +0.0), and the tree runs over the chains in s_a
// [FS_CHAINS][FS_FIN_COLS].  The sum of column j0 + cc is returned to the threads of chain 0; the others get a value that means nothing.
// Barriers: ALL FS_FIN_THREADS threads of the workgroup call it, in uniform control flow.  It ends without a barrier -- a chain-0 thread
// returns the cell it wrote itself in the last step -- so the threads of chain 0 may still be reading the cells of chain 1 when the
// others return: a __syncthreads() has to pass before s_a is written again, by a next call or by anything else.
__device__ __forceinline__ double fs_finish_cols(const double* __restrict__ part, int64_t P, int nq, int j0, double* s_a) {
#pragma clang fp contract(off)
  const int q = (int)threadIdx.x / FS_FIN_COLS, cc = (int)threadIdx.x % FS_FIN_COLS;
  const int j = j0 + cc;
  double a = 0.0;
  if (j < nq)
    for (int64_t p = q; p < P; p += FS_CHAINS) a = a + part[p * nq + j];
  s_a[q * FS_FIN_COLS + cc] = a;
  for (int h = FS_CHAINS / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (q < h) s_a[q * FS_FIN_COLS + cc] = s_a[q * FS_FIN_COLS + cc] + s_a[(q + h) * FS_FIN_COLS + cc];
  }
  return s_a[q * FS_FIN_COLS + cc];
}
