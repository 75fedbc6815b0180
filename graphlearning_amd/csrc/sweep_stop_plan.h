// The stop test of the Poisson sweeps as the host sees it (sweep_core.hip: glx_sweep_tail), one definition each: the value of a row of
// sharded maxima, the bits of the start value, and the walk that decides from the read-back rows at which sweep count every group
// stops (the `while` of reference graphlearning/ssl.py:667).  B groups of which the first `used` run; the single form is B = used = 1.
// No HIP header: tests/sweep_stop_host.cpp compiles it for the host and tests/test_sweep_stop_host.py plays the device against it.
#pragma once
#include <cstdint>
#include <cstring>

static const int SWEEP_TAIL_CHUNK = 16;    // conditional sweeps launched between two read-backs of the stop values
static const int SWEEP_MAX_GROUPS = 32;

// The stop value of one group at one sweep count: the kernel keeps max|deg w - vinf| as `nshards` atomic maxima of fp64 bit patterns
// (non-negative values and the NaN marker order like uint64: NaN sorts above +inf).
static inline double stop_value(const unsigned long long* shards, int nshards) {
  unsigned long long m = 0;
  for (int k = 0; k < nshards; ++k) m = shards[k] > m ? shards[k] : m;
  double d;
  memcpy(&d, &m, 8);
  return d;
}

// err0 = max|v_0 - vinf| as the first shard of row 0 (min_iter = 0: the test in front of the first sweep).  A NaN becomes the
// positive quiet NaN: still a NaN, and as a bit pattern above every number, so it ends the loop like `nan > 1/n`.
static inline unsigned long long stop_bits(double err0) {
  if (err0 != err0) return 0x7ff8000000000000ull;
  unsigned long long u;
  memcpy(&u, &err0, 8);
  return u;
}

struct StopWalk {
  int B = 1, used = 0, head = 0, max_iter = 0;
  double thresh = 0.0;
  int T[SWEEP_MAX_GROUPS] = {0};             // per group: sweeps of the run; -1 while it is still running
  char stopped[SWEEP_MAX_GROUPS] = {0};      // per group: did the stop test end it (not max_iter)?

  // the state behind the head: min(min_iter, max_iter) unconditional sweeps have been enqueued; idle groups have T = 0
  void start(int B_, int used_, int min_iter, int max_iter_, double thresh_) {
    B = B_;
    used = used_;
    head = min_iter < max_iter_ ? min_iter : max_iter_;
    max_iter = max_iter_;
    thresh = thresh_;
    for (int b = 0; b < B; ++b) {
      T[b] = b < used ? -1 : 0;
      stopped[b] = 0;
    }
  }
  bool running() const {
    for (int b = 0; b < used; ++b)
      if (T[b] < 0) return true;
    return false;
  }
  // ssl.py:667 at sweep count t, for the groups still running.  row = err[t]: B x nshards maxima.  `!(e > thresh)`: a NaN stops.
  void test(int t, const unsigned long long* row, int nshards) {
    for (int b = 0; b < used; ++b)
      if (T[b] < 0 && !(stop_value(row + (size_t)b * nshards, nshards) > thresh)) {
        T[b] = t;
        stopped[b] = 1;
      }
  }
  // the chunk launched at sweep count t is sweeps t .. chunk_end(t) - 1; they write rows t + 1 .. chunk_end(t) of err
  int chunk_end(int t) const { return max_iter < t + SWEEP_TAIL_CHUNK ? max_iter : t + SWEEP_TAIL_CHUNK; }
  // groups never stopped ran to max_iter (the value at t = max_iter is never compared, ssl.py:667); returns the largest T
  int finish() {
    int T_max = head;
    for (int b = 0; b < used; ++b) {
      if (T[b] < 0) T[b] = max_iter;
      T_max = T[b] > T_max ? T[b] : T_max;
    }
    return T_max;
  }
  // values compared with the threshold: err[head .. head + count)
  int tested_count(int b) const {
    const int c = T[b] - head + (stopped[b] ? 1 : 0);
    return c > 0 ? c : 0;
  }
  // Which ping-pong buffer holds u_T.  Sweep t reads buffer t & 1 and writes the other (the head starts from buffer 0), and sweep
  // T_max - 1 is the last one that wrote anything: launches behind a group's stop copy it forward or return at once.  (Counting
  // from a chunk's first sweep t0 with cur0 = t0 & 1, cur0 ^ ((T - t0) & 1) is the same number.)
  static int parity(int T_max) { return T_max & 1; }
};
