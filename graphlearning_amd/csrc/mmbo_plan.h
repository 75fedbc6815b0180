// What the host derives and decides for the multiclass MBO learner (glx_mmbo_solve, mmbo.hip): the checks of the caller's arrays, the
// per-vertex training label, the factors of the eigenvalues, the assignment of rows to partial sums, and mmbo_host_reference, which
// walks the documented order on the host, reductions included.  No HIP header: tests/test_mmbo_host.py builds it on
// the host (tests/mmbo_plan_host.cpp).
//
// The iteration (reference ssl.py:989-996; Garcia-Cardona et al. 2014).  X is (n, m) row-major, vals (m), k classes.  With
// h = dt / Ns, c0 = h * mu and d[j] = 1 / (1 + h * vals[j]), each rounded once on the host, one of the T * Ns steps forms, with every
// operation rounded on its own (no fused multiply-add):
//     u[i, c]  per vertex i and class c:  1 or 0 from the vertex's label   (the first step, and the first step after a projection)
//                                         sum over j = 0 .. m-1 in order, from +0.0, of Z[c, j] * X[i, j]            (otherwise)
//     b[i, c]  = u[i, c]                                  off the training vertices
//              = u[i, c] - c0 * (u[i, c] - K[i, c])       on them, K the one-hot of the training label (a vertex listed twice: the last)
//     y[i, j]  = X[i, j] * d[j]                           (the eigenvalue factor goes on X as it is read, as the reference's Y = X V does)
//     Z[c, j]  = sum over i of b[i, c] * y[i, j]          in the reduction order below
// The projection after every Ns steps is label[i] = the first c with the largest u[i, c] (a later entry wins only if it is strictly
// greater; a NaN never wins over entry 0), from the u of the Z that the Ns-th step left.  The only per-vertex state is the label: the
// first pass of the next outer iteration forms u from Z, decides and records the label and goes on with its one-hot, and one last
// pass decides the labels of outer iteration T.  u is never stored.
//
// The reduction order.  Rows [64 p, 64 p + 64) form partial p whatever k and m are.  Inside a partial every (c, j) is ONE CHAIN over the
// partial's rows in ascending order from +0.0 -- not the halving tree of fs_tree64: a tree over 64 rows wants 64 k m doubles side by
// side (2 MiB at the cap), a chain wants one register per (c, j).  Rows past n are not added.  The partials of a (c, j) are finished
// in the order of fixed_sum.h (fs_finish).  Nothing depends on which workgroup ends first.
//
// Caps: k <= 256, m <= 256, k * m <= MMBO_CAP = 4096 (Z in LDS: 32 KiB and a pad), n * m, T * n and partials * k * m at most 2^31.
#pragma once
#include "csr_plan.h"
#include "fixed_sum.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>

static const int MMBO_ROWS = FS_ROWS;         // rows per partial sum
static const int MMBO_SUB_MIN = 8;            // rows a workgroup of the pass holds in LDS at a time, at least (mmbo_sub_rows)
static const int MMBO_LDS_BYTES = 48 << 10;   // what the pass's LDS may take before the rows held at a time are halved
static const int MMBO_THREADS = 256;          // threads of the pass
static const int MMBO_MAX_K = 256;
static const int MMBO_MAX_M = 256;
static const int MMBO_CAP = 4096;             // k * m at most
static const int64_t MMBO_MAX_STEPS = 1ll << 24;

struct MmboPlan {
  std::vector<int32_t> tl;                    // (n) the training label of a vertex (the last one that lists it), -1 elsewhere
  std::vector<double> d;                      // (m) 1 / (1 + h * vals[j])
  double c0 = 0;                              // (dt / Ns) * mu
  int64_t P = 0;                              // partials: fs_partials(n)
};

inline void mmbo_factors(int m, const double* vals, int64_t Ns, double dt, double mu, double* c0, double* d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double h = dt / (double)Ns;
  *c0 = h * mu;
  for (int j = 0; j < m; ++j) {
    const double t = h * vals[j];
    const double s = 1.0 + t;
    d[j] = 1.0 / s;
  }
}

// 0, or a message in `msg` and: 1 sizes, 2 Ns, T or T * Ns, 3 dt or mu not finite, 4 a training vertex out of range, 5 a training
// label outside [0, k), 6 a start label outside [0, k), 7 X, vals or a factor 1 / (1 + (dt / Ns) vals[j]) not finite, 8 unsupported
// (k or m above 256, k * m above MMBO_CAP, n * m, T * n or partials * k * m above 2^31)
inline int mmbo_validate(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                         const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu, char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll || m < 1 || k < 1 || ntrain < 0) {
    snprintf(msg, cap, "bad sizes (n=%lld m=%d k=%d training vertices=%lld; n at most 2^31 - 1)", (long long)n, m, k, (long long)ntrain);
    return 1;
  }
  if (Ns < 1 || T < 1 || Ns > MMBO_MAX_STEPS || T > MMBO_MAX_STEPS || T * Ns > MMBO_MAX_STEPS) {
    snprintf(msg, cap, "Ns=%lld or T=%lld below 1, or T * Ns above 2^24", (long long)Ns, (long long)T);
    return 2;
  }
  if (!std::isfinite(dt) || !std::isfinite(mu)) {
    snprintf(msg, cap, "dt=%g or mu=%g not finite", dt, mu);
    return 3;
  }
  const int64_t P = fs_partials(n);
  if (k > MMBO_MAX_K || m > MMBO_MAX_M || (int64_t)k * m > MMBO_CAP || n * (int64_t)m > (1ll << 31) || T * n > (1ll << 31) ||
      P * (int64_t)k * m > (1ll << 31)) {
    snprintf(msg, cap, "k=%d classes or m=%d columns (at most %d and %d), k * m = %d (at most %d), or n * m, T * n or partials * k * m above 2^31",
             k, m, MMBO_MAX_K, MMBO_MAX_M, k * m, MMBO_CAP);
    return 8;
  }
  for (int64_t q = 0; q < ntrain; ++q) {
    if (const int bad = csr_check_vertex(ind[q], n, 4, "training", msg, cap)) return bad;
    if (lab[q] < 0 || lab[q] >= k) {
      snprintf(msg, cap, "training label %d outside [0, %d)", lab[q], k);
      return 5;
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (lab0[i] < 0 || lab0[i] >= k) {
      snprintf(msg, cap, "start label %d of vertex %lld outside [0, %d)", lab0[i], (long long)i, k);
      return 6;
    }
  for (int64_t q = 0; q < n * (int64_t)m; ++q)
    if (!std::isfinite(X[q])) {
      snprintf(msg, cap, "X[%lld, %lld] = %g is not finite", (long long)(q / m), (long long)(q % m), X[q]);
      return 7;
    }
  double c0, d[MMBO_MAX_M];
  mmbo_factors(m, vals, Ns, dt, mu, &c0, d);
  for (int j = 0; j < m; ++j)
    if (!std::isfinite(vals[j]) || !std::isfinite(d[j])) {
      snprintf(msg, cap, "vals[%d] = %g or its factor 1 / (1 + (dt / Ns) vals) = %g is not finite", j, vals[j], d[j]);
      return 7;
    }
  return 0;
}

inline void mmbo_make_plan(int64_t n, int m, const double* vals, int64_t ntrain, const int32_t* ind, const int32_t* lab, int64_t Ns, double dt,
                           double mu, MmboPlan* out) {
  MmboPlan& P = *out;
  P.d.assign((size_t)m, 0.0);
  mmbo_factors(m, vals, Ns, dt, mu, &P.c0, P.d.data());
  P.tl.assign((size_t)n, -1);
  for (int64_t q = 0; q < ntrain; ++q) P.tl[ind[q]] = lab[q];
  P.P = fs_partials(n);
}

// LDS doubles of the pass with `sub` rows held at a time: Z with its rows padded to an odd length, the rows' X, the rows' u
inline size_t mmbo_lds_doubles(int k, int m, int sub) { return (size_t)k * (m | 1) + (size_t)sub * m + (size_t)sub * k; }
// The rows of its partial a workgroup of the pass holds in LDS at a time: 64, halved while the LDS would exceed MMBO_LDS_BYTES, not
// below 8 (52 KiB at the cap).  No part of the arithmetic: the chain of a (c, j) runs over the rows in ascending order either way.
inline int mmbo_sub_rows(int k, int m) {
  int sub = MMBO_ROWS;
  while (sub > MMBO_SUB_MIN && mmbo_lds_doubles(k, m, sub) * 8 > (size_t)MMBO_LDS_BYTES) sub /= 2;
  return sub;
}

// first row and rows of partial p
inline void mmbo_partial_rows(int64_t n, int64_t p, int64_t* i0, int* rows) {
  *i0 = p * MMBO_ROWS;
  *rows = (int)(n - *i0 < MMBO_ROWS ? n - *i0 : MMBO_ROWS);
}

// what a pass does before it adds up
enum MmboMode {
  MMBO_START = 0,                             // u from the labels handed in
  MMBO_PLAIN = 1,                             // u from Z
  MMBO_PROJECT = 2,                           // u from Z, the label decided and recorded, then u from the label
  MMBO_LABELS = 3                             // u from Z, the label decided and recorded, nothing added up
};
// the pass of step g (0-based) of T * Ns
constexpr int mmbo_mode(int64_t g, int64_t Ns) { return g == 0 ? MMBO_START : (g % Ns == 0 ? MMBO_PROJECT : MMBO_PLAIN); }

// the first index of the largest entry
inline int mmbo_argmax(const double* u, int k) {
  int best = 0;
  for (int c = 1; c < k; ++c)
    if (u[c] > u[best]) best = c;
  return best;
}

// ---- the documented order on the host: what the device must equal bit for bit ------------------------------------------------------

// one pass: labels (read by MMBO_START; written by MMBO_PROJECT and MMBO_LABELS), Z (k, m) -> part (P, k m).  gap (or null): lowered
// to the smallest difference between the largest and the second largest u of a vertex this pass decided (k >= 2).
inline void mmbo_host_pass(const MmboPlan& plan, int64_t n, int m, int k, const double* X, int mode, const int32_t* lab_in, int32_t* lab_out,
                           const double* Z, double* part, double* gap) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int km = k * m;
  std::vector<double> acc((size_t)km), u((size_t)k), y((size_t)m);
  for (int64_t p = 0; p < plan.P; ++p) {
    int64_t i0;
    int rows;
    mmbo_partial_rows(n, p, &i0, &rows);
    for (int q = 0; q < km; ++q) acc[q] = 0.0;
    for (int r = 0; r < rows; ++r) {
      const int64_t i = i0 + r;
      const double* x = X + i * m;
      int label = mode == MMBO_START ? lab_in[i] : -1;
      if (mode != MMBO_START)
        for (int c = 0; c < k; ++c) {
          double s = 0.0;
          for (int j = 0; j < m; ++j) {
            const double pr = Z[c * m + j] * x[j];
            s = s + pr;
          }
          u[c] = s;
        }
      if (mode == MMBO_PROJECT || mode == MMBO_LABELS) {
        label = mmbo_argmax(u.data(), k);
        lab_out[i] = label;
        if (gap && k >= 2) {
          double second = -std::numeric_limits<double>::infinity();
          for (int c = 0; c < k; ++c)
            if (c != label && u[c] > second) second = u[c];
          const double g = u[label] - second;
          if (!(g >= *gap)) *gap = g;
        }
      }
      if (mode == MMBO_LABELS) continue;
      if (mode != MMBO_PLAIN)
        for (int c = 0; c < k; ++c) u[c] = c == label ? 1.0 : 0.0;
      const int32_t tl = plan.tl[i];
      if (tl >= 0)
        for (int c = 0; c < k; ++c) {
          const double K = c == tl ? 1.0 : 0.0;
          const double t1 = u[c] - K;
          const double t2 = plan.c0 * t1;
          u[c] = u[c] - t2;
        }
      for (int j = 0; j < m; ++j) y[j] = x[j] * plan.d[j];
      for (int c = 0; c < k; ++c)
        for (int j = 0; j < m; ++j) {
          const double pr = u[c] * y[j];
          acc[c * m + j] = acc[c * m + j] + pr;
        }
    }
    if (mode != MMBO_LABELS)
      for (int q = 0; q < km; ++q) part[p * km + q] = acc[q];
  }
}

// The whole call on the host: hist (T, n) the labels after every outer iteration, Zlast (k, m) the Z of the last step, *min_gap (or
// null) the smallest top-two gap over all T projections (+inf when k = 1).
inline void mmbo_host_reference(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                                const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu, int32_t* hist, double* Zlast,
                                double* min_gap) {
  MmboPlan plan;
  mmbo_make_plan(n, m, vals, ntrain, ind, lab, Ns, dt, mu, &plan);
  const int km = k * m;
  std::vector<double> part((size_t)plan.P * km), Z((size_t)km, 0.0);
  double gap = std::numeric_limits<double>::infinity();
  for (int64_t g = 0; g < T * Ns; ++g) {
    const int mode = mmbo_mode(g, Ns);
    mmbo_host_pass(plan, n, m, k, X, mode, lab0, mode == MMBO_PROJECT ? hist + (g / Ns - 1) * n : nullptr, Z.data(), part.data(), &gap);
    fs_finish(part.data(), plan.P, km, Z.data());
  }
  mmbo_host_pass(plan, n, m, k, X, MMBO_LABELS, nullptr, hist + (T - 1) * n, Z.data(), nullptr, &gap);
  for (int q = 0; q < km; ++q) Zlast[q] = Z[q];
  if (min_gap) *min_gap = gap;
}
