// csrc/sweep_stop_plan.h on the host, behind a C interface for tests/test_sweep_stop_host.py:
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.
#include "sweep_stop_plan.h"

extern "C" {

// out[0 .. 2): sweeps per tail chunk, the largest number of groups
void ssw_constants(int* out) {
  out[0] = SWEEP_TAIL_CHUNK;
  out[1] = SWEEP_MAX_GROUPS;
}

double ssw_stop_value(const unsigned long long* shards, int nshards) { return stop_value(shards, nshards); }
unsigned long long ssw_stop_bits(double err0) { return stop_bits(err0); }

StopWalk* ssw_new() { return new StopWalk(); }
void ssw_free(StopWalk* w) { delete w; }
void ssw_start(StopWalk* w, int B, int used, int min_iter, int max_iter, double thresh) { w->start(B, used, min_iter, max_iter, thresh); }
int ssw_head(const StopWalk* w) { return w->head; }
int ssw_running(const StopWalk* w) { return w->running() ? 1 : 0; }
void ssw_test(StopWalk* w, int t, const unsigned long long* row, int nshards) { w->test(t, row, nshards); }
int ssw_chunk_end(const StopWalk* w, int t) { return w->chunk_end(t); }
int ssw_finish(StopWalk* w) { return w->finish(); }
int ssw_T(const StopWalk* w, int b) { return w->T[b]; }
int ssw_stopped(const StopWalk* w, int b) { return w->stopped[b]; }
int ssw_tested_count(const StopWalk* w, int b) { return w->tested_count(b); }
int ssw_parity(int T_max) { return StopWalk::parity(T_max); }

}  // extern "C"
