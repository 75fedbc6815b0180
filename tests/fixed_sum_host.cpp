// csrc/fixed_sum.h on the host, behind a C interface for tests/test_fixed_sum_host.py (tests/fixed_sum_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.
#include "fixed_sum.h"

extern "C" {

// out[0 .. 3): rows per partial, chains, columns a finishing workgroup reduces at a time
void fs_host_constants(int* out) {
  out[0] = FS_ROWS;
  out[1] = FS_CHAINS;
  out[2] = FS_FIN_COLS;
}

int64_t fs_host_partials(int64_t n) { return fs_partials(n); }

// the tree over v[0 .. live) and 64 - live rows of +0.0
double fs_host_tree64(const double* v, int live) {
  double a[FS_ROWS];
  for (int r = 0; r < FS_ROWS; ++r) a[r] = r < live ? v[r] : 0.0;
  return fs_tree64(a);
}

double fs_host_tree_dot(const double* x, const double* y, int64_t n, int64_t p) { return fs_tree_dot(x, y, n, p); }

void fs_host_finish(const double* part, int64_t P, int nq, double* S) { fs_finish(part, P, nq, S); }
}
