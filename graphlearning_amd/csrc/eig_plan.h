// What the host derives and decides for the thick-restart Lanczos eigensolver (glx_eig_*, eig.hip): the checks of the caller's arrays,
// the basis size, the memory estimate, and EigHost, which walks every device operation in the documented order on the
// host, reductions included.  No HIP header: tests/test_eig_host.py builds it on the host (tests/eig_plan_host.cpp) and runs the same
// Python driver (graphlearning_amd/_eig.py) on it that runs on the device object.
//
// The operator.  A is a symmetric canonical CSR matrix (n rows, columns strictly ascending inside a row, values finite, a stored
// diagonal is legal); the method works on B = A A, so that the k largest SINGULAR values of A are found.  The basis is column-major:
// Lanczos vector c is the n contiguous doubles V[c n .. c n + n); there are m + 1 columns.
//
// One Lanczos step j works on the columns 0 .. j, every operation rounded on its own (no fused multiply-add):
//   1. t = A v_j, w = A t: each row adds its stored entries in order, from +0.0, of val[e] * x[col[e]];
//   2. h_c = v_c . w for c = 0 .. j in the reduction order of fixed_sum.h: the 64 rows of a partial by fs_tree64 (fs_tree_dot), the
//      partials of a column by fs_finish;
//   3. w_i <- w_i - h_c * v_c[i] for c = 0, 1, .. j in that order, product and difference rounded separately;
//   4. 2 and 3 once more, giving g; alpha_j = h_j + g_j, beta_j = sqrt(w . w) in the same reduction order, v_{j+1}[i] = w_i / beta_j.
// Orthonormalising column j is 2 - 4 without the operator: w = v_j, the columns 0 .. j - 1, v_j <- w / sqrt(w . w).
// The rotation V[:, :keep] <- V[:, :rows] Y adds, per element, the products V[i, c] * Y[c, q] over c = 0 .. rows - 1 in ascending
// order from +0.0; then V[:, keep] <- V[:, rows].
#pragma once
#include "csr_plan.h"
#include "fixed_sum.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

static const int EIG_MAX_M = 513;          // widest basis: 2 * EIG_MAX_K + 1
static const int EIG_MAX_K = 256;          // columns handed out at once at most
#ifndef EIG_WG_PARTIALS
#define EIG_WG_PARTIALS 1                  // 64-row partials (wavefronts) per workgroup of the streaming kernels, 1 .. 16: the mapping is
#endif                                     // not part of the contract (measured: 1 and 2 ahead of 4 and 8 by 3-5 %, 16 behind by 20 %)
static const int EIG_ROT_ROWS = 8;         // rows of the basis a workgroup of the rotation holds in LDS (8 * 513 doubles)

// ARPACK's ncv as scipy's svds chooses it: min(max(2 k + 1, 20), n)
inline int64_t eig_basis_size(int64_t n, int64_t k) {
  int64_t m = 2 * k + 1 > 20 ? 2 * k + 1 : 20;
  return m < n ? m : n;
}

// device bytes of a solver object at its peak: the m + 1 basis columns, w and t, the CSR arrays, the partial sums of m + 1 columns
// and the scalars.  The rotation works in place out of LDS: no scratch of the basis' size.
inline int64_t eig_device_bytes(int64_t n, int64_t nnz, int64_t m) {
  return (m + 1 + 2) * n * 8 + (n + 1) * 8 + nnz * 12 + fs_partials(n) * (m + 1) * 8 + (int64_t)EIG_MAX_M * EIG_MAX_M * 8 + 8 * (m + 1) * 8;
}

// 0, or a message in `msg` and: 1 sizes, 2 row pointers, 3 a column index out of range, 4 a row with columns not strictly ascending,
// 6 a value that is not finite, 8 m outside [1, min(n, EIG_MAX_M)]
inline int eig_validate(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int64_t m, char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll) {
    snprintf(msg, cap, "bad size n=%lld (1 .. 2^31 - 1)", (long long)n);
    return 1;
  }
  if (m < 1 || m > n || m > EIG_MAX_M) {
    snprintf(msg, cap, "basis size m=%lld outside [1, min(n, %d)] (n=%lld)", (long long)m, EIG_MAX_M, (long long)n);
    return 8;
  }
  const int64_t M = row_ptr[n];
  if (row_ptr[0] != 0 || M < 0 || M > 0x7fffffffll) {
    snprintf(msg, cap, "row pointers run from %lld to %lld, expected 0 to at most 2^31 - 1", (long long)row_ptr[0], (long long)M);
    return 2;
  }
  return csr_walk(n, M, row_ptr, col, 2, 3, 4, msg, cap, [&](int64_t, int64_t e) {
    if (std::isfinite(val[e])) return 0;
    snprintf(msg, cap, "value %g of entry %lld is not finite", val[e], (long long)e);
    return 6;
  });
}

// ---- the documented order on the host: what the device must equal bit for bit ------------------------------------------------------

// y = A x
inline void eig_h_spmv(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, const double* x, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const double pr = val[e] * x[col[e]];
      s = s + pr;
    }
    y[i] = s;
  }
}

// h[c] = v_c . w for c < count; part: fs_partials(n) * count doubles of scratch
inline void eig_h_dots(int64_t n, const double* V, int count, const double* w, double* part, double* h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (count < 1) return;
  const int64_t P = fs_partials(n);
  for (int64_t p = 0; p < P; ++p)
    for (int c = 0; c < count; ++c) part[p * count + c] = fs_tree_dot(V + (int64_t)c * n, w, n, p);
  fs_finish(part, P, count, h);
}

// w_i <- w_i - h[c] * v_c[i], c ascending
inline void eig_h_update(int64_t n, const double* V, int count, const double* h, double* w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int64_t i = 0; i < n; ++i) {
    double wi = w[i];
    for (int c = 0; c < count; ++c) {
      const double pr = h[c] * V[(int64_t)c * n + i];
      wi = wi - pr;
    }
    w[i] = wi;
  }
}

// sqrt(w . w); part: fs_partials(n) doubles of scratch
inline double eig_h_norm(int64_t n, const double* w, double* part) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int64_t P = fs_partials(n);
  double s;
  for (int64_t p = 0; p < P; ++p) part[p] = fs_tree_dot(w, w, n, p);
  fs_finish(part, P, 1, &s);
  return std::sqrt(s);
}

// a solver object on the host: the operations of glx_eig_* with loops in place of the kernels.  Every member returns 0 or the number
// of the argument that is out of range.
struct EigHost {
  int64_t n = 0;
  int m = 0;
  std::vector<int64_t> row_ptr;
  std::vector<int32_t> col;
  std::vector<double> val, V, w, t, part, h, g;

  void create(int64_t n_, const int64_t* rp, const int32_t* c, const double* v, int m_) {
    n = n_;
    m = m_;
    row_ptr.assign(rp, rp + n + 1);
    col.assign(c, c + rp[n]);
    val.assign(v, v + rp[n]);
    V.assign((size_t)(m + 1) * n, 0.0);
    w.assign((size_t)n, 0.0);
    t.assign((size_t)n, 0.0);
    part.assign((size_t)fs_partials(n) * (m + 1), 0.0);
    h.assign((size_t)m + 1, 0.0);
    g.assign((size_t)m + 1, 0.0);
  }
  int set_column(int j, const double* x) {
    if (j < 0 || j > m) return 2;
    memcpy(&V[(size_t)j * n], x, (size_t)n * 8);
    return 0;
  }
  // items 2 - 4 on w against the columns [0, count); the new column goes to `dst`; returns beta
  double orthogonalise(int count, int dst, double* alpha_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    eig_h_dots(n, V.data(), count, w.data(), part.data(), h.data());
    eig_h_update(n, V.data(), count, h.data(), w.data());
    eig_h_dots(n, V.data(), count, w.data(), part.data(), g.data());
    eig_h_update(n, V.data(), count, g.data(), w.data());
    if (alpha_out) *alpha_out = h[count - 1] + g[count - 1];
    const double beta = eig_h_norm(n, w.data(), part.data());
    double* out = &V[(size_t)dst * n];
    for (int64_t i = 0; i < n; ++i) out[i] = w[i] / beta;
    return beta;
  }
  int orthonormalize(int j, double* norm) {
    if (j < 0 || j > m) return 2;
    memcpy(w.data(), &V[(size_t)j * n], (size_t)n * 8);
    *norm = orthogonalise(j, j, nullptr);
    return 0;
  }
  int run(int j0, int j1, double* alpha, double* beta) {
    if (j0 < 0 || j0 >= j1 || j1 > m) return 2;
    for (int j = j0; j < j1; ++j) {
      eig_h_spmv(n, row_ptr.data(), col.data(), val.data(), &V[(size_t)j * n], t.data());
      eig_h_spmv(n, row_ptr.data(), col.data(), val.data(), t.data(), w.data());
      beta[j - j0] = orthogonalise(j + 1, j + 1, &alpha[j - j0]);
    }
    return 0;
  }
  // Y (rows, keep) row-major
  int rotate(const double* Y, int rows, int keep) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (rows < 1 || rows > m || keep < 1 || keep > rows) return 3;
    std::vector<double> row((size_t)rows);
    for (int64_t i = 0; i < n; ++i) {
      for (int c = 0; c < rows; ++c) row[c] = V[(size_t)c * n + i];
      for (int q = 0; q < keep; ++q) {
        double s = 0.0;
        for (int c = 0; c < rows; ++c) {
          const double pr = row[c] * Y[(size_t)c * keep + q];
          s = s + pr;
        }
        V[(size_t)q * n + i] = s;
      }
    }
    if (keep != rows) memcpy(&V[(size_t)keep * n], &V[(size_t)rows * n], (size_t)n * 8);
    return 0;
  }
  // out (j1 - j0, n): column j0 first
  int get_columns(int j0, int j1, double* out) const {
    if (j0 < 0 || j0 >= j1 || j1 > m + 1) return 2;
    memcpy(out, &V[(size_t)j0 * n], (size_t)(j1 - j0) * n * 8);
    return 0;
  }
};
