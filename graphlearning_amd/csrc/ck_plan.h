// What the host derives and decides for the centered-kernel learner (glx_ck_solve, ck.hip): the checks of the caller's arrays, the
// column sums c = W^T 1 and row sums d = W 1, the assignment of rows to partial sums, the chunk schedule with its stop decision, and
// ck_host_reference, which walks the documented order on the host, reductions included.  No HIP header:
// tests/test_ck_host.py builds it on the host (tests/ck_plan_host.cpp).
//
// The iteration.  With C x = x - mean(x) column by column, C W C u = W u - d (x) m - 1 (x) yb where m = invn * (1^T u) and
// yb = invn * (c^T u - sc * m), invn = 1 / n rounded once and sc = sum(c).  One pass forms, per (vertex i, column b) and with every
// operation rounded on its own (no fused multiply-add):
//     s  = sum over the row's stored entries in order, from +0.0, of W[e] * u[col[e], b]
//     w  = inva * ((s - d[i] * m[b]) - yb[b]) - u[i, b];      w = 0 on a training row
//     u' = u[i, b] + w
// and leaves, per partial of FS_ROWS consecutive rows, the sums of u' and of c[i] * u' and the integer maximum of the bit patterns of
// |w| (non-negative doubles order like their bit patterns, and a NaN's pattern lies above every number's: a NaN reaches the slot).
//
// The reduction order is the one of fixed_sum.h: the 64 rows of a partial by fs_tree64, the partials of a column by fs_finish.
//
// The power iteration is the same pass with one column: x is e at first and the unnormalised product afterwards, e_i = x_i / nrm
// formed where it is read, w = (W e - d * m) - yb, and the partials of e.w, e.e, w.w, 1.w and c.w give l = |e.w / e.e|,
// nrm' = sqrt(w.w), m' = invn * (1.w / nrm'), yb' = invn * (c.w / nrm' - sc * m').
//
// The stop is the reference's `while err > tol` with err = 1 at first: iteration q (1-based) is the last one iff !(err_q > tol).
// Every iteration has a slot; a new chunk's slots hold NaN except slot 0, which carries the last slot of the chunk before (1.0 at
// the very start).  A pass and its finishing kernel first look at the slot before theirs and do nothing when !(slot > tol): after the
// stop every later slot stays NaN, which stops as well, whatever tol is.
#pragma once
#include "csr_plan.h"
#include "fixed_sum.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

static const int CK_TILE = 16;             // columns per workgroup of the pass at most (FS_ROWS * CK_TILE threads)
static const int CK_CHUNK = 64;            // iterations enqueued between two reads of the error slots
static const int CK_MAX_COLS = 256;
static const int64_t CK_MAX_IT = 1ll << 24;

struct CkPlan {
  std::vector<double> c, d;                // (n) column and row sums of W
  std::vector<int32_t> lab;                // (n) the row of `val` a training vertex starts from (the last one that lists it), -1 elsewhere
  double sc = 0, invn = 0;
  int64_t P = 0;                           // partials: fs_partials(n)
  int ntiles = 0, ct = 0;                  // column tiles of the pass and the widest tile's columns
};

// the column tiles of the pass: the tile rule of csr_plan.h with at most CK_TILE columns each
inline void ck_tiles(int k, int* ntiles, int* ct) { col_tiles(k, CK_TILE, ntiles, ct); }
inline void ck_tile(int k, int t, int* c0, int* cols) { col_tile(k, CK_TILE, t, c0, cols); }

// 0, or a message in `msg` and: 1 sizes, 2 row pointers, 3 a column index out of range, 4 a row with columns not strictly ascending,
// 5 a stored diagonal entry, 6 a weight that is not finite, 7 a training vertex out of range, 8 power_it, alpha_frac or max_it,
// 9 unsupported (k above CK_MAX_COLS, n * k above 2^31)
inline int ck_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                       int64_t power_it, double alpha_frac, int64_t max_it, char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll || M < 0 || M > 0x7fffffffll || m < 0 || k < 1) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%lld m=%lld k=%d; n and M at most 2^31 - 1)", (long long)n, (long long)M, (long long)m, k);
    return 1;
  }
  if (k > CK_MAX_COLS || n * (int64_t)k > (1ll << 31)) {
    snprintf(msg, cap, "k=%d columns (at most %d) or n * k = %lld values (at most 2^31)", k, CK_MAX_COLS, (long long)(n * (int64_t)k));
    return 9;
  }
  if (power_it < 1 || power_it > CK_MAX_IT || !(max_it >= 1 && max_it <= CK_MAX_IT) || !std::isfinite(alpha_frac)) {
    snprintf(msg, cap, "power_it=%lld or max_it=%lld outside [1, 2^24], or alpha_frac=%g not finite", (long long)power_it, (long long)max_it,
             alpha_frac);
    return 8;
  }
  const int bad = csr_walk(n, M, row_ptr, col, 2, 3, 4, msg, cap, [&](int64_t i, int64_t e) {
    if (col[e] == i) {
      snprintf(msg, cap, "row %lld stores its diagonal entry (the caller removes the diagonal)", (long long)i);
      return 5;
    }
    if (!std::isfinite(W[e])) {
      snprintf(msg, cap, "weight %g of entry %lld is not finite", W[e], (long long)e);
      return 6;
    }
    return 0;
  });
  return bad ? bad : csr_check_vertices(ind, m, n, 7, "training", msg, cap);
}

inline void ck_make_plan(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                         CkPlan* out) {
  CkPlan& P = *out;
  P.c.assign((size_t)n, 0.0);
  P.d.assign((size_t)n, 0.0);
  for (int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      s = s + W[e];
      P.c[col[e]] = P.c[col[e]] + W[e];
    }
    P.d[i] = s;
  }
  double sc = 0.0;
  for (int64_t j = 0; j < n; ++j) sc = sc + P.c[j];
  P.sc = sc;
  P.invn = 1.0 / (double)n;
  P.lab = csr_label_rows(n, m, ind);
  P.P = fs_partials(n);
  ck_tiles(k, &P.ntiles, &P.ct);
}

// the start of the fixed-point iteration: u0 = val on the training rows, zero elsewhere, and its (P, 2 k) partials (sums of u0, then
// of c * u0) without forming u0 where no training row lies
inline void ck_start_partials(const CkPlan& plan, int64_t n, int k, const double* val, double* part) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a[FS_ROWS], b[FS_ROWS];
  for (int64_t p = 0; p < plan.P; ++p) {
    const int64_t i0 = p * FS_ROWS;
    bool any = false;
    for (int r = 0; r < FS_ROWS && i0 + r < n; ++r) any = any || plan.lab[i0 + r] >= 0;
    for (int c = 0; c < k; ++c) {
      double s1 = 0.0, s2 = 0.0;
      if (any) {
        for (int r = 0; r < FS_ROWS; ++r) {
          const int64_t i = i0 + r;
          const double v = (i < n && plan.lab[i] >= 0) ? val[(int64_t)plan.lab[i] * k + c] : 0.0;
          a[r] = v;
          b[r] = i < n ? plan.c[i] * v : 0.0;
        }
        s1 = fs_tree64(a);
        s2 = fs_tree64(b);
      }
      part[p * 2 * k + c] = s1;
      part[p * 2 * k + k + c] = s2;
    }
  }
}

// m and yb of a column from its two finished sums
inline void ck_means(double S1, double Sc, double sc, double invn, double* mean, double* yb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = invn * S1;
  const double t = sc * m;
  const double y = Sc - t;
  *mean = m;
  *yb = invn * y;
}

// the start of the power iteration: nrm = 1 and the means of e itself
inline void ck_power_start(const CkPlan& plan, int64_t n, const double* e, double* mean, double* yb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  std::vector<double> part((size_t)plan.P * 2);
  double a[FS_ROWS], b[FS_ROWS];
  for (int64_t p = 0; p < plan.P; ++p) {
    for (int r = 0; r < FS_ROWS; ++r) {
      const int64_t i = p * FS_ROWS + r;
      a[r] = i < n ? e[i] : 0.0;
      b[r] = i < n ? plan.c[i] * e[i] : 0.0;
    }
    part[p * 2] = fs_tree64(a);
    part[p * 2 + 1] = fs_tree64(b);
  }
  double S[2];
  fs_finish(part.data(), plan.P, 2, S);
  ck_means(S[0], S[1], plan.sc, plan.invn, mean, yb);
}

// has the iteration whose slot this is been the last one (or did none run after it)?
constexpr bool ck_stopped(double slot, double tol) { return !(slot > tol); }

// the slots (chunk + 1) of a new chunk: slot 0 <- the last slot of the chunk before (1.0: the reference's err before the loop),
// the others <- NaN.  The device does the same with a kernel.
inline void ck_slots_next(double* slots, int chunk, int prev_len, bool first) {
  const double carry = first ? 1.0 : slots[prev_len];
  for (int r = 1; r <= chunk; ++r) slots[r] = std::numeric_limits<double>::quiet_NaN();
  slots[0] = carry;
}

// The chunk schedule and the joint stop: iteration q is the last iff !(err_q > tol).  (GlxStops decides per column with
// `e < tol && q > after`; this stop is joint and compares the other way round.)
struct CkStops {
  double tol;
  int64_t max_it, it = 0, T = 0;
  int prev_len = 0;
  bool done;
  CkStops(double tol_, int64_t max_it_) : tol(tol_), max_it(max_it_), done(ck_stopped(1.0, tol_)) {}
  // iterations of the next chunk; 0: stopped, or max_it iterations ran without a stop (capped())
  int next_len(int chunk) const {
    if (done || it >= max_it) return 0;
    return (int)(max_it - it < chunk ? max_it - it : chunk);
  }
  bool capped() const { return !done; }
  // errs: the slots 1 .. len of the chunk that ran; hist (or null): err of iteration q at hist[q - 1] while q <= cap
  void decide(const double* errs, int len, double* hist, int64_t cap) {
    for (int r = 0; r < len; ++r) {
      if (hist && it + r < cap) hist[it + r] = errs[r];
      if (ck_stopped(errs[r], tol)) {
        T = it + r + 1;
        done = true;
        break;
      }
    }
    if (!done) it += len;
    prev_len = len;
  }
};

// ---- the documented order on the host: what the device must equal bit for bit ------------------------------------------------------

// one power pass: x, nrm, mean, yb -> xout (the unnormalised product) and S[5] = e.w, e.e, w.w, 1.w, c.w
inline void ck_host_power_pass(const CkPlan& plan, int64_t n, const int64_t* row_ptr, const int32_t* col, const double* W, const double* x,
                               double nrm, double mean, double yb, double* xout, double* S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  std::vector<double> part((size_t)plan.P * 5);
  double a[5][FS_ROWS];
  for (int64_t p = 0; p < plan.P; ++p) {
    for (int r = 0; r < FS_ROWS; ++r) {
      const int64_t i = p * FS_ROWS + r;
      for (int j = 0; j < 5; ++j) a[j][r] = 0.0;
      if (i >= n) continue;
      double s = 0.0;
      for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
        const double ej = x[col[e]] / nrm;
        const double pr = W[e] * ej;
        s = s + pr;
      }
      const double ei = x[i] / nrm;
      const double t1 = plan.d[i] * mean;
      const double y1 = s - t1;
      const double w = y1 - yb;
      xout[i] = w;
      a[0][r] = ei * w;
      a[1][r] = ei * ei;
      a[2][r] = w * w;
      a[3][r] = w;
      a[4][r] = plan.c[i] * w;
    }
    for (int j = 0; j < 5; ++j) part[p * 5 + j] = fs_tree64(a[j]);
  }
  fs_finish(part.data(), plan.P, 5, S);
}

// what the finishing kernel of a power pass leaves
inline void ck_power_finish(const CkPlan& plan, const double* S, double* l, double* nrm, double* mean, double* yb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *l = std::fabs(S[0] / S[1]);
  *nrm = std::sqrt(S[2]);
  const double s1 = S[3] / *nrm, s2 = S[4] / *nrm;
  ck_means(s1, s2, plan.sc, plan.invn, mean, yb);
}

// one pass of the fixed-point iteration: uin, mean[k], yb[k] -> uout, the (P, 2 k) partials and err
inline double ck_host_pass(const CkPlan& plan, int64_t n, const int64_t* row_ptr, const int32_t* col, const double* W, int k, double inva,
                           const double* uin, const double* mean, const double* yb, double* uout, double* part) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  uint64_t emax = 0;
  std::vector<double> a((size_t)2 * k * FS_ROWS);
  for (int64_t p = 0; p < plan.P; ++p) {
    for (int r = 0; r < FS_ROWS; ++r) {
      const int64_t i = p * FS_ROWS + r;
      for (int c = 0; c < k; ++c) {
        double v1 = 0.0, v2 = 0.0;
        if (i < n) {
          double s = 0.0;
          for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const double pr = W[e] * uin[(int64_t)col[e] * k + c];
            s = s + pr;
          }
          const double ui = uin[i * k + c];
          const double t1 = plan.d[i] * mean[c];
          const double y1 = s - t1;
          const double y2 = y1 - yb[c];
          const double sv = inva * y2;
          double w = sv - ui;
          if (plan.lab[i] >= 0) w = 0.0;
          const double un = ui + w;
          uout[i * k + c] = un;
          v1 = un;
          v2 = plan.c[i] * un;
          const uint64_t bits = __builtin_bit_cast(uint64_t, std::fabs(w));
          emax = bits > emax ? bits : emax;
        }
        a[(size_t)c * FS_ROWS + r] = v1;
        a[(size_t)(k + c) * FS_ROWS + r] = v2;
      }
    }
    for (int j = 0; j < 2 * k; ++j) part[p * 2 * k + j] = fs_tree64(&a[(size_t)j * FS_ROWS]);
  }
  return __builtin_bit_cast(double, emax);
}

// The whole call on the host with the chunked schedule of the device (chunk: iterations between two stop decisions): u (n, k), l, T,
// err_hist[0 .. min(T, cap)).  Returns 0, or 1 when max_it iterations ran without a stop.
inline int ck_host_reference(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                             const double* val, const double* e, int64_t power_it, double alpha_frac, double tol, int64_t max_it, int chunk,
                             double* u, double* l_out, int64_t* T_out, double* err_hist, int64_t cap) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  CkPlan plan;
  ck_make_plan(n, row_ptr, col, W, k, m, ind, &plan);
  // power iteration
  std::vector<double> xa(e, e + n), xb((size_t)n);
  double nrm = 1.0, mean, yb, l = 0.0, S5[5];
  ck_power_start(plan, n, e, &mean, &yb);
  for (int64_t q = 0; q < power_it; ++q) {
    ck_host_power_pass(plan, n, row_ptr, col, W, xa.data(), nrm, mean, yb, xb.data(), S5);
    ck_power_finish(plan, S5, &l, &nrm, &mean, &yb);
    xa.swap(xb);
  }
  const double alpha = alpha_frac * l;
  const double inva = 1.0 / alpha;
  // fixed-point iteration, two buffers: iteration q reads buf[(q - 1) & 1] and writes buf[q & 1]
  std::vector<double> buf[2], part((size_t)plan.P * 2 * k), S((size_t)2 * k), mk((size_t)k), yk((size_t)k);
  buf[0].assign((size_t)n * k, 0.0);
  buf[1].assign((size_t)n * k, 0.0);
  for (int64_t i = 0; i < n; ++i)
    if (plan.lab[i] >= 0)
      for (int c = 0; c < k; ++c) buf[0][i * k + c] = val[(int64_t)plan.lab[i] * k + c];
  ck_start_partials(plan, n, k, val, part.data());
  fs_finish(part.data(), plan.P, 2 * k, S.data());
  for (int c = 0; c < k; ++c) ck_means(S[c], S[k + c], plan.sc, plan.invn, &mk[c], &yk[c]);
  std::vector<double> slots((size_t)chunk + 1);
  CkStops stops(tol, max_it);
  bool first = true;
  for (int len; (len = stops.next_len(chunk)) > 0;) {
    ck_slots_next(slots.data(), chunk, stops.prev_len, first);
    first = false;
    for (int r = 1; r <= len; ++r) {
      if (ck_stopped(slots[r - 1], tol)) continue;           // launches after the stop change nothing
      const int64_t q = stops.it + r;
      slots[r] = ck_host_pass(plan, n, row_ptr, col, W, k, inva, buf[(q - 1) & 1].data(), mk.data(), yk.data(), buf[q & 1].data(), part.data());
      fs_finish(part.data(), plan.P, 2 * k, S.data());
      for (int c = 0; c < k; ++c) ck_means(S[c], S[k + c], plan.sc, plan.invn, &mk[c], &yk[c]);
    }
    stops.decide(slots.data() + 1, len, err_hist, cap);
  }
  *l_out = l;
  *T_out = stops.done ? stops.T : stops.it;
  const std::vector<double>& res = buf[*T_out & 1];
  for (int64_t q = 0; q < n * k; ++q) u[q] = res[q];
  return stops.capped() ? 1 : 0;
}
