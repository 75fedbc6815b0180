// csrc/mmbo_plan.h on the host, behind a C interface for tests/test_mmbo_host.py (tests/mmbo_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  With -DMMBO_PLAN_MAIN it is a stand-alone program that walks a small problem
// through every function (for a host sanitizer run: g++ -fsanitize=address,undefined -DMMBO_PLAN_MAIN).
#include "mmbo_plan.h"
#include <cstring>

extern "C" {

int mmbo_host_validate(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                       const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu) {
  char msg[256];
  return mmbo_validate(n, m, X, vals, lab0, ntrain, ind, lab, k, Ns, T, dt, mu, msg, sizeof msg);
}

// 0, or minus what mmbo_validate answered
int mmbo_host_solve(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                    const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu, int32_t* hist, double* Zlast, double* min_gap) {
  char msg[256];
  const int rc = mmbo_validate(n, m, X, vals, lab0, ntrain, ind, lab, k, Ns, T, dt, mu, msg, sizeof msg);
  if (rc) return -rc;
  mmbo_host_reference(n, m, X, vals, lab0, ntrain, ind, lab, k, Ns, T, dt, mu, hist, Zlast, min_gap);
  return 0;
}

// rows of its partial a workgroup of the pass holds in LDS at a time, and the bytes of LDS that takes
int mmbo_host_sub_rows(int k, int m, int64_t* lds_bytes) {
  const int sub = mmbo_sub_rows(k, m);
  *lds_bytes = (int64_t)(mmbo_lds_doubles(k, m, sub) * 8);
  return sub;
}

// out[0 .. 2 P): first row and rows of every partial; returns P
int64_t mmbo_host_partials(int64_t n, int64_t* out, int64_t cap) {
  const int64_t P = (n + MMBO_ROWS - 1) / MMBO_ROWS;
  for (int64_t p = 0; p < P && p < cap; ++p) {
    int rows;
    mmbo_partial_rows(n, p, &out[2 * p], &rows);
    out[2 * p + 1] = rows;
  }
  return P;
}
}

#ifdef MMBO_PLAN_MAIN
int main() {
  // 150 vertices (three partials, the last one short), 5 columns, 3 classes, the step modes of Ns = 3, T = 2 and of Ns = 1
  const int64_t n = 150;
  const int m = 5, k = 3;
  std::vector<double> X((size_t)n * m), vals((size_t)m), Z((size_t)k * m), Z2((size_t)k * m);
  std::vector<int32_t> lab0((size_t)n), hist((size_t)3 * n), hist2((size_t)3 * n);
  for (int64_t i = 0; i < n; ++i) {
    lab0[i] = (int32_t)((i * 7) % k);
    for (int j = 0; j < m; ++j) X[i * m + j] = 0.05 * (double)(((i + 3) * (j + 2) * 31) % 41) - 1.0;
  }
  for (int j = 0; j < m; ++j) vals[j] = 0.3 * j;
  const int32_t ind[4] = {0, 64, 149, 64}, lab[4] = {0, 1, 2, 2};
  if (mmbo_host_validate(n, m, X.data(), vals.data(), lab0.data(), 4, ind, lab, k, 3, 2, 0.15, 50.0)) return 1;
  int64_t rows[6];
  if (mmbo_host_partials(n, rows, 3) != 3 || rows[4] != 128 || rows[5] != 22) return 2;
  double gap;
  if (mmbo_host_solve(n, m, X.data(), vals.data(), lab0.data(), 4, ind, lab, k, 3, 2, 0.15, 50.0, hist.data(), Z.data(), &gap)) return 3;
  if (mmbo_host_solve(n, m, X.data(), vals.data(), lab0.data(), 4, ind, lab, k, 3, 2, 0.15, 50.0, hist2.data(), Z2.data(), nullptr)) return 3;
  if (memcmp(hist.data(), hist2.data(), (size_t)2 * n * 4) || memcmp(Z.data(), Z2.data(), (size_t)k * m * 8)) return 4;
  if (mmbo_host_solve(n, m, X.data(), vals.data(), lab0.data(), 0, nullptr, nullptr, k, 1, 3, 0.15, 50.0, hist2.data(), Z2.data(), nullptr)) return 5;
  for (int64_t q = 0; q < 3 * n; ++q)
    if (hist2[q] < 0 || hist2[q] >= k) return 6;
  if (mmbo_host_validate(n, m, X.data(), vals.data(), lab0.data(), 4, ind, lab, k, 0, 2, 0.15, 50.0) != 2) return 7;
  printf("ok gap %g labels %d %d Z %.17g\n", gap, hist[n], hist[2 * n - 1], Z[0]);
  return 0;
}
#endif
