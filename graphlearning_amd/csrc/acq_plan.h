// What the host derives and decides for the acquisition functions of active learning (glx_acq_*, acq.hip): the checks of the caller's
// arrays, the tiling rule, and the complete arithmetic -- acq_host_compute, acq_host_update, acq_host_greedy walk the documented order
//  on the host.  No device header: tests/test_al_host.py builds it on the host (tests/acq_plan_host.cpp).
//
// The state (reference active_learning.py:285-317, spectral truncation): V (n, M) row-major, the rows v_i being the vertices in the
// truncated eigenbasis, C (M, M) row-major, gamma2.  Every operation is rounded on its own (no fused multiply-add); every sum is ONE
// CHAIN in ascending index from +0.0.  For a vertex i with v = V[i, :]:
//     w[a]  = sum over b = 0 .. M-1 of C[a, b] * v[b]                      a = 0 .. M-1
//     d     = sum over a of v[a] * w[a]
//     s1    = sum over a of w[a]               s2 = sum over a of w[a] * w[a]
//     den   = gamma2 + d
//     VAR    (sqrt(s2) * sqrt(s2)) / den       (the reference's np.linalg.norm(..) ** 2.: sqrt is correctly rounded, so are both roundings)
//     SIGMA  (s1 * s1) / den
//     MC     (unc * sqrt(s2)) / den            (the reference's unc_terms * col_norms / diag_terms, left to right)
//     MCVAR  (unc * (sqrt(s2) * sqrt(s2))) / den
// A value that is not finite is returned as it is.  The rank-one step of a query k, v = V[k, :], with w as above:
//     ip = sum over a of v[a] * w[a];  den = gamma2 + ip;  C[a, b] = C[a, b] - (w[a] * w[b]) / den      (numpy's C -= np.outer(w, w) / den)
// The greedy design (VAR, SIGMA): b rounds on a copy of C.  A round evaluates every candidate position whose vertex was not chosen
// before and takes the first maximum: acq_better -- a larger value wins, a NaN wins over every number (numpy's argmax), equal values
// (or two NaN) go to the smaller position in cand.  The rule is a total order, so the result does not depend on how the positions are
// grouped.  A round whose maximum is not finite ends the call.  The chosen VERTEX leaves the candidates (every position that lists it).
//
// Caps: 1 <= M <= 256 (the cap of eigen_decomp's k), 1 <= n <= 2^31 - 1, at most 2^31 - 1 candidates.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define ACQ_FN __host__ __device__ inline
#else
#define ACQ_FN inline
#endif

static const int ACQ_MAX_M = 256;
static const int ACQ_THREADS = 256;            // threads of a workgroup of the pass: ACQ_THREADS / acq_tile_rows(M) per candidate of its tile
static const int ACQ_TILE_MAX = 64;            // candidates of a tile at most: their last step runs in one wavefront
static const int ACQ_LDS_BYTES = 56 << 10;     // what a tile's rows of V and of w = C v may take in LDS before the tile is halved
static const int ACQ_UPD_THREADS = 256;        // threads of the single workgroup that applies rank-one steps
static const int ACQ_UPD_LDS_M = 80;           // the update holds C in LDS up to this M (80 * 81 * 8 = 51 840 bytes), in L2 beyond
enum AcqKind { ACQ_VAR = 0, ACQ_SIGMA = 1, ACQ_MC = 2, ACQ_MCVAR = 3 };

// candidates per workgroup of the pass: 64, halved while their rows of V and of w (each padded to an odd length) exceed ACQ_LDS_BYTES
// (8 at M = 256).  No part of the arithmetic: a candidate's value depends on nothing but its own row, and its sums are chains.
inline size_t acq_tile_lds_bytes(int R, int M) { return 2 * (size_t)R * (size_t)(M | 1) * 8; }
inline int acq_tile_rows(int M) {
  int R = ACQ_TILE_MAX;
  while (R > 1 && acq_tile_lds_bytes(R, M) > (size_t)ACQ_LDS_BYTES) R /= 2;
  return R;
}
inline size_t acq_pass_lds_bytes(int M) { return acq_tile_lds_bytes(acq_tile_rows(M), M); }
inline bool acq_update_in_lds(int M) { return M <= ACQ_UPD_LDS_M; }
inline size_t acq_update_lds_bytes(int M) { return acq_update_in_lds(M) ? (size_t)M * (size_t)(M | 1) * 8 : 0; }

// 0, or a message in `msg` and: 1 sizes, 2 an entry of V or C or gamma2 not finite, 8 unsupported (M above 256, n above 2^31 - 1)
inline int acq_validate_state(int64_t n, int M, const double* V, const double* C, double gamma2, char* msg, size_t cap) {
  if (n < 1 || M < 1) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%d)", (long long)n, M);
    return 1;
  }
  if (M > ACQ_MAX_M || n > 0x7fffffffll) {
    snprintf(msg, cap, "M=%d columns (at most %d) or n=%lld above 2^31 - 1", M, ACQ_MAX_M, (long long)n);
    return 8;
  }
  if (!std::isfinite(gamma2)) {
    snprintf(msg, cap, "gamma2=%g is not finite", gamma2);
    return 2;
  }
  for (int64_t q = 0; q < n * (int64_t)M; ++q)
    if (!std::isfinite(V[q])) {
      snprintf(msg, cap, "V[%lld, %lld] = %g is not finite", (long long)(q / M), (long long)(q % M), V[q]);
      return 2;
    }
  for (int q = 0; q < M * M; ++q)
    if (!std::isfinite(C[q])) {
      snprintf(msg, cap, "C[%d, %d] = %g is not finite", q / M, q % M, C[q]);
      return 2;
    }
  return 0;
}

// 0, or: 3 a kind outside the four (or, for the greedy design, not VAR or SIGMA), 4 a position outside [0, n), 5 sizes
inline int acq_validate_cand(int64_t n, int kind, bool greedy, const int32_t* cand, int64_t nc, char* msg, size_t cap) {
  if (kind < ACQ_VAR || kind > ACQ_MCVAR || (greedy && kind > ACQ_SIGMA)) {
    snprintf(msg, cap, "kind %d%s", kind, greedy ? " (the greedy design takes VAR = 0 and SIGMA = 1: the others look at labels)" : " outside 0 .. 3");
    return 3;
  }
  if (nc < 0 || nc > 0x7fffffffll) {
    snprintf(msg, cap, "%lld candidates (0 .. 2^31 - 1)", (long long)nc);
    return 5;
  }
  for (int64_t p = 0; p < nc; ++p)
    if (cand[p] < 0 || cand[p] >= n) {
      snprintf(msg, cap, "position %d (entry %lld) outside [0, %lld)", cand[p], (long long)p, (long long)n);
      return 4;
    }
  return 0;
}

// the vertices the positions name, each counted once
inline int64_t acq_distinct(const int32_t* cand, int64_t nc) {
  std::vector<int32_t> s(cand, cand + nc);
  std::sort(s.begin(), s.end());
  return (int64_t)(std::unique(s.begin(), s.end()) - s.begin());
}

// the value from the three sums
ACQ_FN double acq_value(int kind, double gamma2, double d, double s1, double s2, double unc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double den = gamma2 + d;
  if (kind == ACQ_SIGMA) {
    const double num = s1 * s1;
    return num / den;
  }
  const double nrm = sqrt(s2);
  if (kind == ACQ_MC) {
    const double num = unc * nrm;
    return num / den;
  }
  const double sq = nrm * nrm;
  if (kind == ACQ_VAR) return sq / den;
  const double num = unc * sq;
  return num / den;
}

// does (val, pos) come before (bval, bpos) in the greedy design's choice?  pos < 0: no candidate
ACQ_FN bool acq_better(double val, int32_t pos, double bval, int32_t bpos) {
  if (pos < 0) return false;
  if (bpos < 0) return true;
  const bool vn = val != val, bn = bval != bval;
  if (vn || bn) return vn && (!bn || pos < bpos);
  return val > bval || (val == bval && pos < bpos);
}

// ---- the documented order on the host: what the device must equal bit for bit ------------------------------------------------------

// the three sums of one row v against C (M, M) with leading dimension M
inline void acq_host_terms(int M, const double* C, const double* v, double* d_out, double* s1_out, double* s2_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double d = 0.0, s1 = 0.0, s2 = 0.0;
  for (int a = 0; a < M; ++a) {
    double w = 0.0;
    for (int b = 0; b < M; ++b) {
      const double pr = C[a * M + b] * v[b];
      w = w + pr;
    }
    const double pd = v[a] * w;
    d = d + pd;
    s1 = s1 + w;
    const double pq = w * w;
    s2 = s2 + pq;
  }
  *d_out = d;
  *s1_out = s1;
  *s2_out = s2;
}

inline double acq_host_one(int kind, int M, const double* C, const double* v, double gamma2, double unc) {
  double d, s1, s2;
  acq_host_terms(M, C, v, &d, &s1, &s2);
  return acq_value(kind, gamma2, d, s1, s2, unc);
}

inline void acq_host_compute(int64_t n, int M, const double* V, const double* C, double gamma2, int kind, const int32_t* cand, int64_t nc,
                             const double* unc, double* vals) {
  (void)n;
  for (int64_t p = 0; p < nc; ++p) vals[p] = acq_host_one(kind, M, C, V + (int64_t)cand[p] * M, gamma2, unc ? unc[p] : 0.0);
}

// C <- C - (w w^T) / (gamma2 + v.w), w = C v
inline void acq_host_rank_one(int M, double* C, const double* v, double gamma2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  std::vector<double> w((size_t)M);
  for (int a = 0; a < M; ++a) {
    double s = 0.0;
    for (int b = 0; b < M; ++b) {
      const double pr = C[a * M + b] * v[b];
      s = s + pr;
    }
    w[a] = s;
  }
  double ip = 0.0;
  for (int a = 0; a < M; ++a) {
    const double pr = v[a] * w[a];
    ip = ip + pr;
  }
  const double den = gamma2 + ip;
  for (int a = 0; a < M; ++a)
    for (int b = 0; b < M; ++b) {
      const double pr = w[a] * w[b];
      const double qt = pr / den;
      C[a * M + b] = C[a * M + b] - qt;
    }
}

inline void acq_host_update(int M, const double* V, double* C, double gamma2, const int32_t* query, int64_t nq) {
  for (int64_t i = 0; i < nq; ++i) acq_host_rank_one(M, C, V + (int64_t)query[i] * M, gamma2);
}

// b rounds on a copy of C: queries (b) <- the chosen POSITIONS in cand, vals (b) <- their values.  0, -1: b < 0 or more rounds than
// distinct vertices, or r + 1 > 0: round r (0-based) had no finite maximum (queries and vals hold the rounds before it).
inline int64_t acq_host_greedy(int64_t n, int M, const double* V, const double* C, double gamma2, int kind, const int32_t* cand, int64_t nc,
                               int64_t b, int32_t* queries, double* vals) {
  if (b < 0 || b > acq_distinct(cand, nc)) return -1;
  std::vector<double> Cs(C, C + (size_t)M * M);
  std::vector<char> removed((size_t)n, 0);
  for (int64_t r = 0; r < b; ++r) {
    double bval = 0.0;
    int32_t bpos = -1;
    for (int64_t p = 0; p < nc; ++p) {
      if (removed[cand[p]]) continue;
      const double val = acq_host_one(kind, M, Cs.data(), V + (int64_t)cand[p] * M, gamma2, 0.0);
      if (acq_better(val, (int32_t)p, bval, bpos)) {
        bval = val;
        bpos = (int32_t)p;
      }
    }
    if (bpos < 0 || !std::isfinite(bval)) return r + 1;
    queries[r] = bpos;
    vals[r] = bval;
    removed[cand[bpos]] = 1;
    acq_host_rank_one(M, Cs.data(), V + (int64_t)cand[bpos] * M, gamma2);
  }
  return 0;
}
