// utils.boundary_statistic (glx_boundary_stat, bstat.hip): the arithmetic, the row-class rule and the argument checks in a form that
// compiles for the host.  No HIP header: tests/bstat_plan_host.cpp is a stand-alone program that runs this file on plain memory and
// is compared bit for bit with the numpy restatement tests/boundary_ref.py.
//
// The reference (utils.py:18-114; Calder, Park, Slepcev, Boundary Estimation from Point Clouds) restated as one walk over the rows of
// a canonical CSR pattern W whose weights are all 1.  Every operation below is rounded on its own (no fused multiply-add), division
// and square root are IEEE.
//   1. a_j = 1.0 / deg_j, deg_j the stored entries of row j.
//   2. raw normal, second order (the rows of W*theta come out of scipy reversed, D - W*theta with the diagonal last):
//        dp_i = chain over the entries of row i in DESCENDING column order, dp = dp + a_j from 0.0;
//        y_c  = chain in ASCENDING column order, y = y + a_j * X[j, c] from 0.0, then y = y + (-dp_i) * X[i, c].
//   3. raw normal, first order (a sorted merge): dp_i = deg_i; the same chain with a = 1.0, the diagonal term (-dp_i) * X[i, c]
//      at the sorted position of column i (before the first neighbour j > i, last if there is none).
//   4. nu[i, c] = y_c / sqrt(np.sum(y * y)), numpy's row sum (npsum_exact.h).
//   5. term of vertex i and member j: V_c = X[i, c] - X[j, c];
//        first order   xd = np.sum(V_c * nu[i, c]);
//        second order  h_c = (nu[i, c] + nu[j, c]) / 2; with cutoff nu2_c = np.sum(nu[i] * nu[j]) > 0 ? h_c : nu[i, c], without
//                      nu2_c = h_c; xd = np.sum(V_c * nu2_c).
//   6. kNN mode: T_i = max of xd over the k members of the list J[i] (self included), NaN if any term is NaN.
//   7. radius mode, maxdeg the longest row.  The reference searches the maxdeg nearest with self counted, so every vertex's list
//      holds its maxdeg - 1 nearest neighbours, and the members outside the ball are masked to 0:
//        a row of fewer than maxdeg - 1 entries gives max(0.0, max of xd over its entries) (a masked-out member is in its list);
//        a row of exactly maxdeg - 1 entries gives the plain maximum of xd over its entries (the list IS the row: no 0);
//        a row of maxdeg entries (a FULL row) drops its farthest entry -- by sqdist_exact, the largest column index among
//        equals -- and adds no 0.  A full row with nothing left (maxdeg = 1) gives -inf.
//      bstat_adds_zero is that rule.
//   8. a zero result is +0.0.
//
// Row classes of the statistic's kernel.  A row's members are dealt to a group of lanes; rows of fewer than BSTAT_WAVE_ROW members
// share a wavefront, BSTAT_SHORT_LANES lanes each, longer rows take the 64 lanes of a wavefront.  No result depends on the
// threshold: the maximum does not depend on the order of its terms.
//
// BSTAT_WAVE_ROW = 512 is EXTRAPOLATED from what profiles/boundary.txt measured on the MI355X (thresholds 1 .. 4096 and "never",
// d = 2), not itself measured:
//   - on the graphs measured the class hardly matters: 70 000 ball-graph rows of 11 .. 83 members 0.194 ms on wavefronts against
//     0.195 ms on 16 lanes, kNN lists of 30 members 0.129 ms against 0.119 ms, ball-graph rows of 46 .. 262 members 0.688 ms against
//     0.701 ms.  Up to 262 members, the longest row measured in numbers, neither class wins by more than a tenth.
//   - one row of 70 000 members beside 70 000 short ones adds 3.9 ms on 16 lanes (24.0 ms against 20.1 ms; the 20 ms are the row's
//     sequential chain of step 2, which the contract fixes): 0.9 us per term and lane.  At that rate a row of 512 members holds
//     its 16 lanes for 32 terms, about 30 us -- a sixth of what all kernels take on 70 000 rows; no longer row should stay there,
//     and on a wavefront it is done in a quarter of that.  Between 262 and 70 000 members nothing was measured.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "csr_plan.h"
#include "npsum_exact.h"
#include "sqdist_tree.h"

#if defined(__HIPCC__)
#define BSTAT_FN __host__ __device__ inline
#else
#define BSTAT_FN inline
#endif

static const int BSTAT_SHORT_LANES = 16;      // lanes per row of the short class (four rows share a wavefront)
static const int BSTAT_WAVE_ROW = 512;        // rows of at least this many members take a whole wavefront
static const int BSTAT_MAX_K = 1024;          // longest list of the kNN mode

// glx_boundary_stat's flags
static const int BSTAT_SECOND_ORDER = 1, BSTAT_CUTOFF = 2;

// step 2 / 3: dp_i.  a (n) holds 1 / deg_j.
BSTAT_FN double bstat_dp(const int32_t* __restrict__ col, int64_t e0, int64_t e1, const double* __restrict__ a, int second_order) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double dp = 0.0;
  if (second_order) {
    for (int64_t e = e1 - 1; e >= e0; --e) dp = dp + a[col[e]];
  } else {
    for (int64_t e = e0; e < e1; ++e) dp = dp + 1.0;
  }
  return dp;
}

// step 2 / 3: the raw normal y_c of vertex i.  X is (n, d) row-major.
BSTAT_FN double bstat_raw(const double* __restrict__ X, int d, const int32_t* __restrict__ col, int64_t e0, int64_t e1,
                          const double* __restrict__ a, int32_t i, int c, double dp, int second_order) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double diag = (-dp) * X[(size_t)i * d + c];
  double y = 0.0;
  if (second_order) {
    for (int64_t e = e0; e < e1; ++e) {
      const int32_t j = col[e];
      const double t = a[j] * X[(size_t)j * d + c];
      y = y + t;
    }
    y = y + diag;
  } else {
    bool placed = false;
    for (int64_t e = e0; e < e1; ++e) {
      const int32_t j = col[e];
      if (!placed && j > i) {
        y = y + diag;
        placed = true;
      }
      const double t = 1.0 * X[(size_t)j * d + c];
      y = y + t;
    }
    if (!placed) y = y + diag;
  }
  return y;
}

// step 4: np.sum(y * y) of one row
// WIDE = false: the caller knows d <= 128, where the row sum is one leaf and needs no stack (the same operations, the same bits)
template <bool WIDE, class Term>
BSTAT_FN double bstat_rowsum(const Term& t, int d) {
  if constexpr (WIDE) return npsum_terms(t, d);
  else return npsum_terms_leaf(t, 0, d);
}
template <bool WIDE = true>
BSTAT_FN double bstat_norm2(const double* __restrict__ y, int d) { return bstat_rowsum<WIDE>(NpsumProduct{y, y}, d); }

// step 5: the term (x_i - x_j) * nu2
struct BstatTerm {
  const double* __restrict__ xi;
  const double* __restrict__ xj;
  const double* __restrict__ ni;
  const double* __restrict__ nj;      // null: nu2 = nu_i
  NPSUM_FN_MEMBER double operator()(int c) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double v = xi[c] - xj[c];
    if (!nj) return v * ni[c];
    const double s = ni[c] + nj[c];
    const double h = s / 2.0;
    return v * h;
  }
};

// step 5: xd of vertex i and member j.  nu is (n, d) row-major.
template <bool WIDE = true>
BSTAT_FN double bstat_term(const double* __restrict__ X, const double* __restrict__ nu, int d, int32_t i, int32_t j, int flags) {
  const double *xi = X + (size_t)i * d, *xj = X + (size_t)j * d, *ni = nu + (size_t)i * d, *nj = nu + (size_t)j * d;
  bool half = (flags & BSTAT_SECOND_ORDER) != 0;
  if (half && (flags & BSTAT_CUTOFF)) half = bstat_rowsum<WIDE>(NpsumProduct{ni, nj}, d) > 0;
  return bstat_rowsum<WIDE>(BstatTerm{xi, xj, ni, half ? nj : nullptr}, d);
}

// step 7: is (sq, j) farther than (best_sq, best_j)?  The largest column index among equal distances.
BSTAT_FN bool bstat_farther(double sq, int32_t j, double best_sq, int32_t best_j) { return sq > best_sq || (sq == best_sq && j > best_j); }

// numpy's maximum over a running pair (mx, nan): NaN wins
BSTAT_FN void bstat_max_in(double xd, double* mx, int* nan) {
  if (xd != xd) *nan = 1;
  else if (xd > *mx) *mx = xd;
}

// step 7: does a row of `len` entries see a masked-out member of the reference's list, i.e. a 0 among its terms?
BSTAT_FN bool bstat_adds_zero(int64_t len, int64_t maxdeg, bool radius_mode) { return radius_mode && len < maxdeg - 1; }

// steps 6 - 8 behind the maximum mx of a row's terms (-inf: none); add_zero: bstat_adds_zero
BSTAT_FN double bstat_finish(double mx, int nan, int add_zero) {
  if (nan) return std::numeric_limits<double>::quiet_NaN();
  if (add_zero && !(mx > 0.0)) mx = 0.0;
  if (mx == 0.0) mx = 0.0;          // -0.0 -> +0.0
  return mx;
}

// lanes a row of `len` members is dealt to
BSTAT_FN int bstat_row_lanes(int64_t len, int wave_row) { return len >= wave_row ? 64 : BSTAT_SHORT_LANES; }

// The argument checks, before anything goes to the device: 0, or `msg` and 1.  indptr (n + 1) / indices: the canonical pattern, no
// empty row; J (n, k) or null: the lists of the kNN mode, every index in [0, n).  *maxdeg <- the longest row.
inline int bstat_check(int64_t n, int d, const int32_t* indptr, const int32_t* indices, int64_t nnz, int k, const int32_t* J,
                       int64_t* maxdeg, char* msg, size_t cap) {
  if (n < 1 || d < 1 || nnz < 0 || n > 0x7fffffff || nnz > 0x7fffffff || (int64_t)n * d > ((int64_t)1 << 38)) {       // (n * d / 256 is a grid size)
    snprintf(msg, cap, "bad sizes (n=%lld d=%d nnz=%lld)", (long long)n, d, (long long)nnz);
    return 1;
  }
  if ((J != nullptr) != (k > 0) || k < 0 || k > BSTAT_MAX_K || k > n) {
    snprintf(msg, cap, "k=%d lists for n=%lld (1 .. min(n, %d), with J)", k, (long long)n, BSTAT_MAX_K);
    return 1;
  }
  std::vector<int64_t> ptr((size_t)n + 1);
  for (int64_t i = 0; i <= n; ++i) ptr[i] = indptr[i];
  int64_t longest = 0;
  const int bad = csr_walk(
      n, nnz, ptr.data(), indices, 1, 1, 1, msg, cap,
      [&](int64_t i, int64_t count) {
        if (count == 0) {
          snprintf(msg, cap, "vertex %lld has no neighbour", (long long)i);
          return 1;
        }
        if (count > longest) longest = count;
        return 0;
      },
      [](int64_t, int64_t) { return 0; }, [](int64_t) { return 0; });
  if (bad) return bad;
  if (J)
    for (int64_t q = 0; q < n * k; ++q)
      if (J[q] < 0 || J[q] >= n) {
        snprintf(msg, cap, "list index %d of vertex %lld out of range", J[q], (long long)(q / k));
        return 1;
      }
  *maxdeg = longest;
  return 0;
}

// The whole computation on the host, in the device's stages.  Returns 0, or 1 + the first vertex whose norm is zero or not finite.
// rows_out[3] (or null): rows of the short class, of the wavefront class, full rows.
inline int64_t bstat_host(int64_t n, int d, const double* X, const int32_t* indptr, const int32_t* indices, int k, const int32_t* J,
                          int flags, double* T, double* nu, int wave_row = BSTAT_WAVE_ROW, int64_t* rows_out = nullptr) {
  const int second = flags & BSTAT_SECOND_ORDER;
  std::vector<double> a((size_t)n), y((size_t)d);
  int64_t maxdeg = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t deg = indptr[j + 1] - indptr[j];
    a[j] = 1.0 / (double)deg;
    if (deg > maxdeg) maxdeg = deg;
  }
  int64_t bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double dp = bstat_dp(indices, indptr[i], indptr[i + 1], a.data(), second);
    for (int c = 0; c < d; ++c) y[c] = bstat_raw(X, d, indices, indptr[i], indptr[i + 1], a.data(), (int32_t)i, c, dp, second);
    const double norm = std::sqrt(d > 128 ? bstat_norm2<true>(y.data(), d) : bstat_norm2<false>(y.data(), d));      // (as the kernels choose)
    if (!(norm > 0.0) || !(norm < std::numeric_limits<double>::infinity())) {
      if (!bad) bad = i + 1;
    }
    for (int c = 0; c < d; ++c) nu[(size_t)i * d + c] = y[c] / norm;
  }
  if (bad) return bad;
  int64_t rows[3] = {0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* mem = J ? J + (size_t)i * k : indices + indptr[i];
    const int64_t len = J ? k : indptr[i + 1] - indptr[i];
    const bool full = !J && len == maxdeg;
    ++rows[bstat_row_lanes(len, wave_row) == 64 ? 1 : 0];
    rows[2] += full;
    int32_t drop = -1;
    if (full) {
      double best = -1.0;
      for (int64_t e = 0; e < len; ++e) {
        const double sq = sqdist_exact(X + (size_t)i * d, X + (size_t)mem[e] * d, d);
        if (bstat_farther(sq, mem[e], best, drop)) {
          best = sq;
          drop = mem[e];
        }
      }
    }
    double mx = -std::numeric_limits<double>::infinity();
    int nan = 0;
    for (int64_t e = 0; e < len; ++e)
      if (mem[e] != drop)
        bstat_max_in(d > 128 ? bstat_term<true>(X, nu, d, (int32_t)i, mem[e], flags) : bstat_term<false>(X, nu, d, (int32_t)i, mem[e], flags),
                     &mx, &nan);
    T[i] = bstat_finish(mx, nan, bstat_adds_zero(len, maxdeg, !J));
  }
  if (rows_out)
    for (int q = 0; q < 3; ++q) rows_out[q] = rows[q];
  return 0;
}
