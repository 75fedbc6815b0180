// What the host derives for dynamic label propagation (glx_dlp_solve, dlp.hip; Wang, Tu and Tsotsos, ICCV 2013; the reference's
// ssl.dynamic_label_propagation, ssl.py:1263-1343): the checks of the caller's arrays, the transpose of P, the training-row map, the
// partial count and workspace sizes, and dlp_host_reference, which walks the documented order on the host.  No HIP
// header: tests/test_dlp_host.py builds it on the host (tests/dlp_plan_host.cpp).
//
// The reference keeps Pt as a dense n x n array and iterates v = P u; u = Pt u; u[train] = K; Pt = P Pt P^T + alpha v v^T + lam I
// (Pt = P at first).  Unrolled, Pt_t X = P (Pt_{t-1} (P^T X)) + alpha v_{t-1} (v_{t-1}^T X) + lam X with Pt_0 X = P X, so the dense
// array is never needed: applying Pt_t to the (n, k) iterate takes 2 t + 1 sparse products and t Gram matrices of size k x k.
//
// The arithmetic contract.  Every operation is rounded on its own: no fused multiply-add, no floating-point atomic; the result is a
// pure function of the arguments.
//   spmm(A, X)[i, b]  a chain over row i's stored entries in stored order, from +0.0, of A[e] * X[col[e], b].
//   P^T               built by the plan from P with a stable counting sort: row j of P^T lists its entries in ascending i.
//   gram(V, X)[c, b]  the fixed_sum.h sum over the vertices i of V[i, c] * X[i, b]: the 64 products of partial p (rows 64 p .. 64 p + 63,
//                     rows past n count as +0.0) are added by fs_tree64, the partials of an entry are finished by fs_finish; k * k
//                     entries, laid out (partials, k * k), entry (c, b) at c * k + b.
//   Start             u_0 is val on the training rows and zero elsewhere; a vertex listed twice takes its last row.
//   Step t = 0 .. T-1
//     v_t = spmm(P, u_t)                                   (only needed for t <= T - 2)
//     Y_0 = u_t, Y_j = spmm(P^T, Y_{j-1}) for j = 1 .. t
//     R_0 = spmm(P, Y_t)                                   (for t = 0 this is v_0, computed once)
//     for s = 0 .. t-1, with X = Y_{t-1-s} and G = gram(v_s, X):
//       g[i, b]       = a chain over c ascending, from +0.0, of v_s[i, c] * G[c, b]
//       R_{s+1}[i, b] = (spmm(P, R_s)[i, b] + alpha * g[i, b]) + lam * X[i, b]
//     u_{t+1} = R_t with the training rows set back to val
//   Nothing skipped   alpha == 0 and lam == 0 take no shortcut, the terms are evaluated as written; no test for non-finite values.
// A fit enqueues T^2 + max(T - 2, 0) sparse passes (the second term: the v_t of the steps 1 .. T-2) and T (T - 1) / 2 Grams.
#pragma once
#include "csr_plan.h"
#include "fixed_sum.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

static const int DLP_TILE = 16;            // columns per workgroup of the sparse pass at most (FS_ROWS * DLP_TILE threads)
static const int DLP_MAX_COLS = 64;        // the Gram has k * k <= 4096 entries: 32 KB of LDS in the pass that applies it
static const int DLP_MAX_T = 64;
static const int64_t DLP_MAX_WORK = 1ll << 30;          // values of workspace: (2 T + 2) n k

struct DlpPlan {
  std::vector<int64_t> tptr;               // (n + 1) row pointers of P^T
  std::vector<int32_t> tcol;               // (M) row j of P^T: the rows i of P that store column j, ascending
  std::vector<double> tval;                // (M)
  std::vector<int32_t> lab;                // (n) the row of `val` a training vertex is set to (the last one that lists it), -1 elsewhere
  int64_t P = 0;                           // partials per Gram entry: fs_partials(n)
  int ntiles = 0, ct = 0;                  // column tiles of the sparse pass (csr_plan.h, at most DLP_TILE columns) and the widest's columns
  int64_t work = 0;                        // values of workspace: (2 T + 2) n k
  int64_t sparse = 0, grams = 0;           // sparse passes and Gram passes of the fit
};

// 0, or a message in `msg` and: 1 sizes, 2 row pointers, 3 a column index out of range, 4 a row with columns not strictly ascending,
// 5 a value that is not finite, 6 a training vertex out of range, 7 T below 1, or alpha or lam not finite, 9 unsupported (k above
// DLP_MAX_COLS, T above DLP_MAX_T, (2 T + 2) n k above DLP_MAX_WORK)
inline int dlp_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m, const int32_t* ind,
                        double alpha, double lam, int64_t T, char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll || M < 0 || M > 0x7fffffffll || m < 0 || k < 1) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%lld m=%lld k=%d; n and M at most 2^31 - 1)", (long long)n, (long long)M, (long long)m, k);
    return 1;
  }
  if (T < 1 || !std::isfinite(alpha) || !std::isfinite(lam)) {
    snprintf(msg, cap, "T=%lld below 1, or alpha=%g or lam=%g not finite", (long long)T, alpha, lam);
    return 7;
  }
  if (k > DLP_MAX_COLS || T > DLP_MAX_T || (2 * T + 2) * n > DLP_MAX_WORK / k) {
    snprintf(msg, cap, "k=%d columns (at most %d), T=%lld steps (at most %d) or (2 T + 2) n k above 2^30 values of workspace", k, DLP_MAX_COLS,
             (long long)T, DLP_MAX_T);
    return 9;
  }
  const int bad = csr_walk(n, M, row_ptr, col, 2, 3, 4, msg, cap, [&](int64_t, int64_t e) {
    if (std::isfinite(P[e])) return 0;
    snprintf(msg, cap, "value %g of entry %lld is not finite", P[e], (long long)e);
    return 5;
  });
  return bad ? bad : csr_check_vertices(ind, m, n, 6, "training", msg, cap);
}

inline void dlp_make_plan(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m,
                          const int32_t* ind, int64_t T, DlpPlan* out) {
  DlpPlan& D = *out;
  // the transpose by a stable counting sort: the rows of P are walked in ascending order, so row j of P^T lists ascending i
  D.tptr.assign((size_t)n + 1, 0);
  for (int64_t e = 0; e < M; ++e) ++D.tptr[(size_t)col[e] + 1];
  for (int64_t j = 0; j < n; ++j) D.tptr[j + 1] += D.tptr[j];
  D.tcol.resize((size_t)M);
  D.tval.resize((size_t)M);
  std::vector<int64_t> at(D.tptr.begin(), D.tptr.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int64_t q = at[col[e]]++;
      D.tcol[q] = (int32_t)i;
      D.tval[q] = P[e];
    }
  D.lab = csr_label_rows(n, m, ind);
  D.P = fs_partials(n);
  col_tiles(k, DLP_TILE, &D.ntiles, &D.ct);
  D.work = (2 * T + 2) * n * k;
  D.sparse = T * T + (T > 2 ? T - 2 : 0);
  D.grams = T * (T - 1) / 2;
}

// ---- the documented order on the host: what the device must equal bit for bit ------------------------------------------------------

// out = spmm(A, X), (n, k) row-major
inline void dlp_host_spmm(int64_t n, const int64_t* ptr, const int32_t* col, const double* A, int k, const double* X, double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int64_t i = 0; i < n; ++i)
    for (int b = 0; b < k; ++b) {
      double s = 0.0;
      for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
        const double pr = A[e] * X[(int64_t)col[e] * k + b];
        s = s + pr;
      }
      out[i * k + b] = s;
    }
}

// G (k, k) = gram(V, X); part: (P, k * k) of work space
inline void dlp_host_gram(int64_t n, int k, const double* V, const double* X, int64_t P, double* part, double* G) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a[FS_ROWS];
  const int kk = k * k;
  for (int64_t p = 0; p < P; ++p)
    for (int c = 0; c < k; ++c)
      for (int b = 0; b < k; ++b) {
        for (int r = 0; r < FS_ROWS; ++r) {
          const int64_t i = p * FS_ROWS + r;
          a[r] = i < n ? V[i * k + c] * X[i * k + b] : 0.0;
        }
        part[p * kk + c * k + b] = fs_tree64(a);
      }
  fs_finish(part, P, kk, G);
}

// The whole call on the host: u (n, k) <- u_T, hist (or null) (T, n, k) <- u_1 .. u_T
inline void dlp_host_reference(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m,
                               const int32_t* ind, const double* val, double alpha, double lam, int64_t T, double* u, double* hist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  DlpPlan plan;
  dlp_make_plan(n, M, row_ptr, col, P, k, m, ind, T, &plan);
  const size_t nk = (size_t)n * k;
  const int64_t* tptr = plan.tptr.data();
  const int32_t* tcol = plan.tcol.data();
  const double* tval = plan.tval.data();
  std::vector<double> cur(nk, 0.0), R(nk), Rn(nk), part((size_t)plan.P * k * k), G((size_t)k * k);
  std::vector<std::vector<double>> V((size_t)(T > 1 ? T - 1 : 0), std::vector<double>(nk)), Y((size_t)T, std::vector<double>(nk));
  for (int64_t i = 0; i < n; ++i)
    if (plan.lab[i] >= 0)
      for (int b = 0; b < k; ++b) cur[i * k + b] = val[(int64_t)plan.lab[i] * k + b];
  for (int64_t t = 0; t < T; ++t) {
    if (t <= T - 2) dlp_host_spmm(n, row_ptr, col, P, k, cur.data(), V[t].data());
    Y[0] = cur;
    for (int64_t j = 1; j <= t; ++j) dlp_host_spmm(n, tptr, tcol, tval, k, Y[j - 1].data(), Y[j].data());
    if (t == 0 && T >= 2) R = V[0];
    else dlp_host_spmm(n, row_ptr, col, P, k, Y[t].data(), R.data());
    for (int64_t s = 0; s < t; ++s) {
      const double* X = Y[t - 1 - s].data();
      const double* v = V[s].data();
      dlp_host_gram(n, k, v, X, plan.P, part.data(), G.data());
      dlp_host_spmm(n, row_ptr, col, P, k, R.data(), Rn.data());
      for (int64_t i = 0; i < n; ++i)
        for (int b = 0; b < k; ++b) {
          double g = 0.0;
          for (int c = 0; c < k; ++c) {
            const double pr = v[i * k + c] * G[(size_t)c * k + b];
            g = g + pr;
          }
          const double ag = alpha * g;
          const double s1 = Rn[i * k + b] + ag;
          const double lx = lam * X[i * k + b];
          Rn[i * k + b] = s1 + lx;
        }
      R.swap(Rn);
    }
    for (int64_t i = 0; i < n; ++i)
      if (plan.lab[i] >= 0)
        for (int b = 0; b < k; ++b) R[i * k + b] = val[(int64_t)plan.lab[i] * k + b];
    cur = R;
    if (hist)
      for (size_t q = 0; q < nk; ++q) hist[(size_t)t * nk + q] = cur[q];
  }
  for (size_t q = 0; q < nk; ++q) u[q] = cur[q];
}
