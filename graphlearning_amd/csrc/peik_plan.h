// The p-eikonal equation  sum_j w_ij (u_i - u_j)_+^p = f_i  off the boundary, u = g on it (graph.peikonal, ssl.peikonal): the
// arithmetic of the synchronous fixed-point rounds of csrc/peik.hip, its argument checks, and the rounds walked on the host
// (peik_host_reference: what the device must equal).  Host only, no HIP include.
//
// The reference's solver (peikonal_fmm_main, c_code/hjsolvers.cpp:342-420) is a fast-marching pass: vertices leave a heap in the order
// of their values, and a vertex j next to the one that leaves is solved again from those of its stored neighbours that already hold a
// value.  The local solve S_j -- the root t of sum_k w_k (t - u_k)_+^p = f over the collected neighbours -- is monotone in every u_k
// and causal (t is above every u_k that takes part in it), the two properties under which the marching order is only one schedule of
//     u_j <- min(u_j, S_j(u)),        u = g on the boundary, +inf elsewhere, neighbours at +inf left out.
// Here every (vertex, problem) does that step at once from the values of the round before, until a round lowers nothing: the fixed
// point of the step, whatever the schedule.  Where it is the marching solver's result (tests/golden/
// make_golden_peikonal.py measures it on every case):
//     p == 1, f > 0, a symmetric pattern: bit for bit;
//     p > 1: to the resolution of the bisection (its bracket depends on which neighbours hold a value when the marching pass solves);
//     p == 1 with f_j == 0: t = fl(fl(u_k w_k) / w_k) can round one unit BELOW u_k, the marching pass never solves a finalised vertex
//       again and stops there, the rounds go on: a few units in the last place lower;
//     p < 1: the reference's bracket [min u + f / deg, max u + f / deg] does not hold the root, its solve returns about min u + f / deg
//       with deg over the neighbours that hold a value at that moment -- not causal: the marching pass's values depend on its
//       schedule, and the fixed point (all neighbours counted) lies well below them;
//     an unsymmetric pattern: the marching pass solves j again only when a vertex that LISTS j leaves the heap, so a vertex that
//       lists others and is listed by nobody keeps u0 there; here it is solved from its row like every other.
//
// Input.  The stored entries of the weight matrix sorted by vertex, in the order of the reference's __ccode_init__: row_ptr (n + 1),
// nbr (M) the neighbour, W (M) the weight, finite and > 0.  f (n) >= 0.  B problems: problem b's boundary vertices are
// bidx[bptr[b] .. bptr[b + 1]) with the values bval; a vertex listed twice takes its last value.  u0 (n): what a vertex holds that
// no boundary reaches (the reference leaves its initial value there).
//
// Start.  u[j, b] = g on problem b's boundary, +inf elsewhere.
// A round, for every (j, b) off the boundary, reading only the values of the round before:
//     collect the entries e of row j with nbr[e] != j (a stored self loop is skipped, hjsolvers.cpp:381) and u_old[nbr[e], b] < inf;
//     none: the value stays;  otherwise t = solve, u_new = t < u_old ? t : u_old.
// Two buffers take turns.  The first round that lowers nothing ends the solve; more than peik_round_cap rounds (2 n + 2 for p == 1)
// are refused (PEIK_ECAP).
// Afterwards a value that is still +inf becomes u0[j].
//
// solve, p == 1 (peikonal_solver_fast, hjsolvers.cpp:265-286).  The collected neighbours in ascending order of (u, position in the
// row) -- a STABLE order of the values, which is what the reference's qsort (glibc's merge sort) leaves --:
//     wsum = u_0 * w_0, deg = w_0, t = (f + wsum) / deg;   while a next neighbour k exists and t > u_k:
//     wsum = wsum + u_k * w_k, deg = deg + w_k, t = (f + wsum) / deg.
// The order comes from repeated scans for the next smallest (u, position): no sort buffer, O(prefix * degree) per solve.
// solve, p != 1 (peikonal_solver, hjsolvers.cpp:229-263), sums in stored order:
//     deg = sum w_k;  inc = f / deg, and inc = pow(inc, 1 / p) if p > 1 (the reference leaves f / deg for p < 1);
//     a = min u + inc, b = max u + inc;  num_bisection_it times: t = (a + b) / 2, op = sum pow(max(t - u_k, 0), p) * w_k,
//     op > f ? b = t : a = t;  the result is (a + b) / 2.
// Every operation is rounded on its own (no fused multiply-add); pow is the library's, so for p != 1 host and device agree to the
// bisection's resolution and for p == 1 bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

static const int PEIK_MAX_COLS = 256;
static const int PEIK_MAX_BISECTION = 128;
static const int64_t PEIK_MAX_VALUES = 1ll << 31;          // n * B
static const int PEIK_ECAP = 12;                           // the rounds went beyond their cap

#if defined(__HIPCC__)
#define PEIK_HD __host__ __device__ __forceinline__
#else
#define PEIK_HD inline
#endif

// The rounds a solve may take before it is refused.  p == 1: a value is final one round after the values it is solved from, so n + 1
// rounds suffice and 2 n + 2 leave a margin.  p != 1: a solve's bracket moves with the largest neighbour, and its result with the
// bracket by up to the bisection's resolution, so behind the rounds that carry the values across the graph come rounds in which
// values fall by that resolution only (28 rounds on a 7-vertex path at p = 2 and 30 halvings, 4 at 60); they get 8 rounds per halving.
inline int64_t peik_round_cap(int64_t n, double p, int num_bisection_it) {
  return 2 * n + 2 + (p == 1 ? 0 : 8 * (int64_t)num_bisection_it);
}

// 0, or a message in `msg` and: 1 sizes or row pointers or a neighbour index out of range, 2 a boundary vertex out of range, 3 an empty
// boundary list (or boundary pointers that do not ascend from 0), 4 a weight that is not finite or <= 0, 5 an f that is negative or not
// finite, 6 a g or u0 that is not finite, 7 p not finite or <= 0, 8 num_bisection_it outside 1 .. 128, 9 B outside 1 .. 256,
// 10 n * B above 2^31
inline int peik_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                         const int64_t* bptr, const int32_t* bidx, const double* bval, double p, int num_bisection_it, const double* u0,
                         char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll || M < 0 || M > 0x7fffffffll) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%lld; n from 1, both at most 2^31 - 1)", (long long)n, (long long)M);
    return 1;
  }
  if (B < 1 || B > PEIK_MAX_COLS) {
    snprintf(msg, cap, "B=%d problems outside 1 .. %d", B, PEIK_MAX_COLS);
    return 9;
  }
  if (n * (int64_t)B > PEIK_MAX_VALUES) {
    snprintf(msg, cap, "n * B = %lld values above the supported 2^31 (split the problems into several calls)", (long long)(n * (int64_t)B));
    return 10;
  }
  if (!(std::isfinite(p) && p > 0)) {
    snprintf(msg, cap, "p=%g is not finite or not positive", p);
    return 7;
  }
  if (num_bisection_it < 1 || num_bisection_it > PEIK_MAX_BISECTION) {
    snprintf(msg, cap, "num_bisection_it=%d outside 1 .. %d", num_bisection_it, PEIK_MAX_BISECTION);
    return 8;
  }
  if (row_ptr[0] != 0 || row_ptr[n] != M) {
    snprintf(msg, cap, "the row pointers do not span the %lld entries", (long long)M);
    return 1;
  }
  for (int64_t j = 0; j < n; ++j)
    if (row_ptr[j] > row_ptr[j + 1]) {
      snprintf(msg, cap, "the row pointers decrease at vertex %lld", (long long)j);
      return 1;
    }
  for (int64_t e = 0; e < M; ++e) {
    if (nbr[e] < 0 || nbr[e] >= n) {
      snprintf(msg, cap, "neighbour index %d of entry %lld out of range", nbr[e], (long long)e);
      return 1;
    }
    if (!(std::isfinite(W[e]) && W[e] > 0)) {
      snprintf(msg, cap, "weight %g of entry %lld is not finite or not positive", W[e], (long long)e);
      return 4;
    }
  }
  for (int64_t j = 0; j < n; ++j) {
    if (!(std::isfinite(f[j]) && f[j] >= 0)) {
      snprintf(msg, cap, "f=%g at vertex %lld is negative or not finite", f[j], (long long)j);
      return 5;
    }
    if (!std::isfinite(u0[j])) {
      snprintf(msg, cap, "u0=%g at vertex %lld is not finite", u0[j], (long long)j);
      return 6;
    }
  }
  if (bptr[0] != 0) {
    snprintf(msg, cap, "the boundary pointers do not start at 0");
    return 3;
  }
  for (int b = 0; b < B; ++b) {
    if (bptr[b + 1] <= bptr[b]) {
      snprintf(msg, cap, "problem %d has an empty boundary list", b);
      return 3;
    }
    for (int64_t q = bptr[b]; q < bptr[b + 1]; ++q) {
      if (bidx[q] < 0 || bidx[q] >= n) {
        snprintf(msg, cap, "boundary vertex %d of problem %d out of range", bidx[q], b);
        return 2;
      }
      if (!std::isfinite(bval[q])) {
        snprintf(msg, cap, "boundary value %g of vertex %d in problem %d is not finite", bval[q], bidx[q], b);
        return 6;
      }
    }
  }
  return 0;
}

// The boundary lists as the device takes them, a vertex listed twice already settled: entry q sets u[vert[q], prob[q]] = val[q], and
// no (vertex, problem) appears twice (the last value of the caller's list is kept).
struct PeikBoundary {
  std::vector<int32_t> vert, prob;
  std::vector<double> val;
};

inline void peik_make_boundary(int64_t n, int B, const int64_t* bptr, const int32_t* bidx, const double* bval, PeikBoundary* out) {
  std::vector<int64_t> at((size_t)n, -1);          // where the problem at hand lists the vertex
  out->vert.clear();
  out->prob.clear();
  out->val.clear();
  for (int b = 0; b < B; ++b) {
    const size_t first = out->vert.size();
    for (int64_t q = bptr[b]; q < bptr[b + 1]; ++q) {
      const int32_t v = bidx[q];
      if (at[v] >= (int64_t)first) {
        out->val[(size_t)at[v]] = bval[q];
        continue;
      }
      at[v] = (int64_t)out->vert.size();
      out->vert.push_back(v);
      out->prob.push_back(b);
      out->val.push_back(bval[q]);
    }
  }
}

// ---- the local solves: one (vertex, problem), the values of the round before at u[nbr * B + b] ------------------------------------

// p == 1.  Returns false when no neighbour holds a value.
PEIK_HD bool peik_solve_fast(const double* u, const int32_t* nbr, const double* W, int64_t e0, int64_t e1, int64_t j, int64_t B, int64_t b,
                             double f, double* t_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double inf = std::numeric_limits<double>::infinity();
  double last_u = 0, wsum = 0, deg = 0, t = 0;
  int64_t last_e = -1;
  for (;;) {
    // the next neighbour in the order (u, position): the smallest pair above (last_u, last_e)
    double nu = inf;
    int64_t ne = -1;
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t kk = nbr[e];
      if (kk == j) continue;
      const double v = u[kk * B + b];
      if (!(v < inf)) continue;
      if (last_e >= 0 && (v < last_u || (v == last_u && e <= last_e))) continue;
      if (ne < 0 || v < nu) {
        nu = v;
        ne = e;
      }
    }
    if (ne < 0) break;
    if (last_e < 0) {
      wsum = nu * W[ne];
      deg = W[ne];
    } else {
      if (!(t > nu)) break;
      const double pr = nu * W[ne];
      wsum = wsum + pr;
      deg = deg + W[ne];
    }
    const double num = f + wsum;
    t = num / deg;
    last_u = nu;
    last_e = ne;
  }
  *t_out = t;
  return last_e >= 0;
}

// p != 1.  POW: the library's pow of the side that compiles this.
PEIK_HD bool peik_solve_bisect(const double* u, const int32_t* nbr, const double* W, int64_t e0, int64_t e1, int64_t j, int64_t B, int64_t b,
                               double f, double p, int num_bisection_it, double* t_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double inf = std::numeric_limits<double>::infinity();
  double mn = 0, mx = 0, deg = 0;
  bool any = false;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t kk = nbr[e];
    if (kk == j) continue;
    const double v = u[kk * B + b];
    if (!(v < inf)) continue;
    if (!any) {
      mn = mx = v;
      any = true;
    }
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    deg = deg + W[e];
  }
  if (!any) return false;
  double inc = f / deg;
  if (p > 1) inc = pow(inc, 1.0 / p);
  double lo = mn + inc, hi = mx + inc;
  for (int it = 0; it < num_bisection_it; ++it) {
    const double s = lo + hi;
    const double t = s / 2.0;
    double op = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t kk = nbr[e];
      if (kk == j) continue;
      const double v = u[kk * B + b];
      if (!(v < inf)) continue;
      const double d = t - v;
      const double c = pow(d > 0 ? d : 0.0, p);
      const double pr = c * W[e];
      op = op + pr;
    }
    if (op > f) hi = t; else lo = t;
  }
  const double s = lo + hi;
  *t_out = s / 2.0;
  return true;
}

// ---- the rounds on the host: what the device must equal (bit for bit for p == 1) ----------------------------------------------------
// u_out (n, B) row-major.  *rounds_out: the rounds run, the idle last one included.  max_rounds: 0, or a cap below the documented one
// (a test hook).  Returns 0, or PEIK_ECAP when the cap is passed (u_out then holds the values of the last round, +inf not replaced).
inline int peik_host_reference(int64_t n, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                               const int64_t* bptr, const int32_t* bidx, const double* bval, double p, int num_bisection_it,
                               const double* u0, int64_t max_rounds, double* u_out, int64_t* rounds_out) {
  const double inf = std::numeric_limits<double>::infinity();
  const size_t total = (size_t)n * (size_t)B;
  std::vector<double> bufs[2] = {std::vector<double>(total, inf), std::vector<double>(total)};
  std::vector<unsigned char> fixed(total, 0);
  PeikBoundary bd;
  peik_make_boundary(n, B, bptr, bidx, bval, &bd);
  for (size_t q = 0; q < bd.vert.size(); ++q) {
    const size_t t = (size_t)bd.vert[q] * B + bd.prob[q];
    bufs[0][t] = bd.val[q];
    fixed[t] = 1;
  }
  int64_t cap = peik_round_cap(n, p, num_bisection_it);
  if (max_rounds > 0 && max_rounds < cap) cap = max_rounds;
  int64_t r = 0;
  int cur = 0, rc = PEIK_ECAP;
  while (r < cap) {
    const double* uo = bufs[cur].data();
    double* un = bufs[1 - cur].data();
    bool lowered = false;
    for (int64_t j = 0; j < n; ++j)
      for (int64_t b = 0; b < B; ++b) {
        const size_t t = (size_t)j * B + b;
        double v = uo[t];
        if (!fixed[t]) {
          double s;
          const bool any = p == 1 ? peik_solve_fast(uo, nbr, W, row_ptr[j], row_ptr[j + 1], j, B, b, f[j], &s)
                                  : peik_solve_bisect(uo, nbr, W, row_ptr[j], row_ptr[j + 1], j, B, b, f[j], p, num_bisection_it, &s);
          if (any && s < v) {
            v = s;
            lowered = true;
          }
        }
        un[t] = v;
      }
    cur = 1 - cur;
    ++r;
    if (!lowered) {
      rc = 0;
      break;
    }
  }
  if (rounds_out) *rounds_out = r;
  const double* res = bufs[cur].data();
  for (int64_t j = 0; j < n; ++j)
    for (int64_t b = 0; b < B; ++b) {
      const double v = res[(size_t)j * B + b];
      u_out[(size_t)j * B + b] = (rc == 0 && !(v < inf)) ? u0[j] : v;
    }
  return rc;
}
