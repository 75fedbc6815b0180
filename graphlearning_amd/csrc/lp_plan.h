// What the host derives and decides for the batched p-Laplace Jacobi iteration (glx_lp_iterate_batch, plaplace.hip): B problems on one
// graph that share the boundary vertices, one per column of val (m, B).  No HIP header: tests/test_plaplace_host.py builds it on the
// host (tests/lp_plan_host.cpp), where a plain loop stands in for the kernel and runs the same chunked two-buffer schedule.
//
// The iteration (c_code/lp_iterate.cpp:35-125).  Two buffers hold (uu, ul) records; iteration `it` reads the first buffer when `it` is
// even and the second when it is odd, and writes the other one.  err of iteration `it` is the largest uu_i - ul_i of the iterate that
// was READ, from 0; the loop ends at the first `it` with err < tol && it > 10, AFTER that iteration has written its output.  The
// caller's arrays are the first buffer (the reference swaps local pointers only), so a column returns
//     U_S        if it stops at an even S (the iterate that was read),
//     U_{S+1}    if it stops at an odd S (the one just written),
//     U_T or U_{T-1} (T even / odd) if it never stops:                 lp_result_iterate.
//
// Stops per column.  Every (iteration, column) has a 64-bit slot that takes the integer maximum of the bit patterns of the positive
// gaps (non-negative doubles order like their bit patterns; a NaN or negative gap leaves the slot alone, like the reference's MAX).
// The host enqueues a chunk of iterations, reads the chunk's slots once and decides per column (LpStops).  On the device a thread of
// iteration `it` finds its column stopped when the slot of iteration it - 1 holds a value below tol and it - 1 > 10 (lp_frozen):
// a stopped column writes nothing, so its later slots stay zero, which is below any tol that can stop at all, and the column stays
// frozen in BOTH buffers through the chunk.  Slots are per chunk: slot 0 carries the last slot of the chunk before (zero for a frozen
// column: still frozen), slots 1 .. len belong to the chunk's iterations.  Device memory does not grow with T.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "glx_stops.h"

static const int LP_BLOCK = 256;           // threads per workgroup of the batched sweep
static const int LP_BATCH_CHUNK = 64;      // iterations enqueued between two reads of the error slots
static const int LP_LDS_COLS = 64;         // up to this many columns a workgroup folds its gaps in LDS before it touches the slots
static const int LP_MAX_COLS = 256;        // columns per call (the cap of the CG solvers)
static const int LP_STOP_AFTER = 10;       // no column stops at an iteration <= this one (lp_iterate.cpp:113)

struct LpPlan {
  std::vector<int64_t> start;     // (n + 1) vertex i's entries are start[i] .. start[i + 1] of the sorted list
  std::vector<double> invdeg;     // (n) alpha / (sum of the vertex's weights, in entry order); alpha / 0 for a vertex without entries
  std::vector<int32_t> bdy;       // (n) the row of val the vertex takes, -1 off the boundary; a vertex listed twice takes its last row
  std::vector<double> hi, lo;     // (B) start values of uu / ul off the boundary: max / min of the column of val
  double alpha = 0, delta = 0, dt = 0;
};

// np.max / np.min of a column: NaN if any value is NaN.  m = 0: the fold's identity (-inf / +inf).
inline void lp_column_range(int64_t m, int B, const double* val, int b, double* hi, double* lo) {
  double h = -std::numeric_limits<double>::infinity(), l = std::numeric_limits<double>::infinity();
  bool nan = false;
  for (int64_t q = 0; q < m; ++q) {
    const double v = val[q * B + b];
    if (v != v) nan = true;
    h = (v > h) ? v : h;
    l = (v < l) ? v : l;
  }
  *hi = nan ? std::numeric_limits<double>::quiet_NaN() : h;
  *lo = nan ? std::numeric_limits<double>::quiet_NaN() : l;
}

// 0, or a message in `msg` and 1 (an argument is out of range: sizes, a neighbour or boundary index) / 2 (unsupported: B above
// LP_MAX_COLS, T above 2^24, n * B above 2^31)
inline int lp_make_plan(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m, const int32_t* ind,
                        const double* val, double p, int64_t T, LpPlan* out, char* msg, size_t cap) {
  if (n < 1 || M < 0 || m < 0 || T < 0 || B < 1) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%lld m=%lld T=%lld B=%d)", (long long)n, (long long)M, (long long)m, (long long)T, B);
    return 1;
  }
  if (B > LP_MAX_COLS) {
    snprintf(msg, cap, "B=%d columns above the supported %d (split the columns into several calls)", B, LP_MAX_COLS);
    return 2;
  }
  if (T > (1ll << 24)) {
    snprintf(msg, cap, "T=%lld above the supported 2^24 iterations", (long long)T);
    return 2;
  }
  if (n > 0x7fffffffll || n * (int64_t)B > (1ll << 31)) {
    snprintf(msg, cap, "n * B = %lld records above the supported 2^31 (split the columns into several calls)", (long long)(n * (int64_t)B));
    return 2;
  }
  LpPlan& P = *out;
  // vertex blocks of the sorted entry list, inverse degrees, largest weight: lp_iterate.cpp:43-64
  P.alpha = 1 / p;
  P.delta = 1 - 2 / p;
  double dt = 0.9 / (P.alpha + 2 * P.delta);
  P.start.assign((size_t)n + 1, 0);
  P.invdeg.assign((size_t)n, 0.0);
  int64_t j = 0;
  for (int64_t i = 0; i < n; ++i) {
    P.start[i] = j;
    double d = 0;
    while (j < M && row[j] == i) {
      if (nbr[j] < 0 || nbr[j] >= n) {
        snprintf(msg, cap, "neighbour index %d out of range", nbr[j]);
        return 1;
      }
      d += W[j];
      ++j;
    }
    P.invdeg[i] = P.alpha / d;
  }
  P.start[n] = j;     // entries past the last vertex's block (unsorted input) are never visited, as in the reference
  double maxw = 0;
  for (int64_t q = 0; q < M; ++q) maxw = (maxw > W[q]) ? maxw : W[q];
  P.dt = dt / maxw;
  P.bdy.assign((size_t)n, -1);
  for (int64_t q = 0; q < m; ++q) {
    if (ind[q] < 0 || ind[q] >= n) {
      snprintf(msg, cap, "boundary index %d out of range", ind[q]);
      return 1;
    }
    P.bdy[ind[q]] = (int32_t)q;
  }
  P.hi.assign((size_t)B, 0.0);
  P.lo.assign((size_t)B, 0.0);
  for (int b = 0; b < B; ++b) lp_column_range(m, B, val, b, &P.hi[b], &P.lo[b]);
  return 0;
}

// has the column of this slot stopped before iteration `it`?  prev: the slot of iteration it - 1
constexpr bool lp_frozen(int64_t it, unsigned long long prev, double tol) {
  return it >= 1 && it - 1 > LP_STOP_AFTER && __builtin_bit_cast(double, prev) < tol;
}

// the slots (chunk + 1, B) of a new chunk: slot 0 <- the last slot of the chunk before (prev_len iterations; 0: the first chunk), the
// others <- 0.  The device does the same with a kernel.
inline void lp_slots_next(unsigned long long* slots, int B, int chunk, int prev_len) {
  for (int b = 0; b < B; ++b) {
    const unsigned long long carry = prev_len > 0 ? slots[(size_t)prev_len * B + b] : 0ull;
    for (int r = 1; r <= chunk; ++r) slots[(size_t)r * B + b] = 0ull;
    slots[b] = carry;
  }
}

// the chunk schedule and stop decision of this iteration: GlxStops with the reference's `it > 10`
struct LpStops : GlxStops {
  LpStops(int B_, int64_t T_, double tol_) : GlxStops(B_, T_, tol_, LP_STOP_AFTER) {}
};

// which iterate U_k the first buffer (what the call returns) holds for a column with this stopping iteration (`stop` = T: never stopped)
inline int64_t lp_result_iterate(int64_t stop, int64_t T) {
  if (stop < T) return (stop & 1) ? stop + 1 : stop;
  return (T & 1) ? T - 1 : T;
}
