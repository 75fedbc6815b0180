// The fixed-order column sum that the single-call solvers share (ck.hip, eig.hip, mmbo.hip): the host side.  The
// device side is fixed_sum_device.h.  No HIP header: the plan headers include this file and are built on the host by the tests
// (tests/fixed_sum_host.cpp tests this one by itself).
//
// The reduction order.  Rows [64 p, 64 p + 64) form partial p whatever the number of columns is; rows past n count as +0.0.  Inside a
// partial the 64 values are added by a halving tree: a[r] += a[r + h] for r < h, h = 32, 16, .. 1 (fs_tree64).  The partials of a
// column are finished by 64 chains -- chain q adds the partials p = q, q + 64, .. in ascending order from +0.0 -- and the same tree
// over the chains (fs_finish).  Nothing depends on which workgroup ends first.  (How the 64 values of a partial come about is the
// solver's own: mmbo.hip adds a partial's rows by one chain, not by the tree, and says so.)
#pragma once
#include <cstdint>

static const int FS_ROWS = 64;             // rows per partial sum
static const int FS_CHAINS = 64;           // chains that finish the partials of a column
static const int FS_FIN_COLS = 16;         // columns a finishing workgroup reduces at a time (FS_CHAINS * FS_FIN_COLS threads)

// partial sums of one column of n rows
inline int64_t fs_partials(int64_t n) { return (n + FS_ROWS - 1) / FS_ROWS; }

// a[0] <- the halving tree over a[0 .. 64)
inline double fs_tree64(double* a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int h = FS_ROWS / 2; h >= 1; h >>= 1)
    for (int r = 0; r < h; ++r) a[r] = a[r] + a[r + h];
  return a[0];
}

// partial p of x . y: the tree over x[i] * y[i], i in [64 p, 64 p + 64), each product rounded on its own
inline double fs_tree_dot(const double* x, const double* y, int64_t n, int64_t p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a[FS_ROWS];
  for (int r = 0; r < FS_ROWS; ++r) {
    const int64_t i = p * FS_ROWS + r;
    a[r] = i < n ? x[i] * y[i] : 0.0;
  }
  return fs_tree64(a);
}

// S[j] for the nq columns of part (P, nq): 64 chains in ascending order, then the tree
inline void fs_finish(const double* part, int64_t P, int nq, double* S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a[FS_CHAINS];
  for (int j = 0; j < nq; ++j) {
    for (int q = 0; q < FS_CHAINS; ++q) {
      double s = 0.0;
      for (int64_t p = q; p < P; p += FS_CHAINS) s = s + part[p * nq + j];
      a[q] = s;
    }
    S[j] = fs_tree64(a);
  }
}
