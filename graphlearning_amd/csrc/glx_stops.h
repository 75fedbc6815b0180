// The host's side of a chunked iteration whose columns stop on their own (plaplace.hip, lip.hip): how long the next chunk is, and
// which column has stopped where once the chunk's error slots were read.  No HIP header: the host tests build it (tests/lp_plan_host.cpp).
//
// The host enqueues a chunk of iterations, reads the chunk's (len, B) slots once and calls decide().  Column b stops at the first
// iteration q whose slot holds a value below tol with q > after -- `err < tol && it > 10` of lp_iterate_main (c_code/lp_iterate.cpp:113),
// `it > 20` of the two lip_iterate loops (:184, :256).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct GlxStops {
  int B;
  int64_t T, it = 0;            // `it`: iterations enqueued so far
  double tol;
  int after;                    // no column stops at an iteration q <= after
  double* hist;                 // optional (T, B): the error of every iteration a column ran, the stopping one included
  int running, prev_len = 0;
  std::vector<int64_t> stop;    // per column: the stopping iteration, -1 while it runs
  GlxStops(int B_, int64_t T_, double tol_, int after_, double* hist_ = nullptr)
      : B(B_), T(T_), tol(tol_), after(after_), hist(hist_), running(B_), stop((size_t)B_, -1) {}
  // iterations of the next chunk (0: every column has stopped or T is reached)
  int next_len(int chunk) const {
    if (running <= 0 || it >= T) return 0;
    return (int)((T - it < chunk) ? T - it : chunk);
  }
  // slots 1 .. len of the chunk that started at iteration `it`, (len, B) row-major
  void decide(const unsigned long long* slots, int len) {
    for (int r = 0; r < len; ++r) {
      const int64_t q = it + r;
      for (int b = 0; b < B; ++b) {
        if (stop[b] >= 0) continue;
        const double e = __builtin_bit_cast(double, slots[(size_t)r * B + b]);
        if (hist) hist[q * B + b] = e;
        if (e < tol && q > after) {
          stop[b] = q;
          --running;
        }
      }
    }
    it += len;
    prev_len = len;
  }
  int64_t iters(int b) const { return stop[b] >= 0 ? stop[b] : T; }
};
