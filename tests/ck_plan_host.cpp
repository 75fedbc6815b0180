// csrc/ck_plan.h on the host, behind a C interface for tests/test_ck_host.py (tests/ck_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  ck_host_solve runs the device's chunked schedule with a plain loop standing in
// for the kernels.  With -DCK_PLAN_MAIN it is a stand-alone program that walks a small graph through every function at the chunk
// lengths 1, 7 and 64 (for a host sanitizer run: g++ -fsanitize=address,undefined -DCK_PLAN_MAIN).
#include "ck_plan.h"
#include <cstring>

extern "C" {

int ck_host_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                     int64_t power_it, double alpha_frac, int64_t max_it) {
  char msg[256];
  return ck_validate(n, M, row_ptr, col, W, k, m, ind, power_it, alpha_frac, max_it, msg, sizeof msg);
}

// out: (first column, columns) per tile of the pass; returns the number of tiles (at most cap are written)
int ck_host_tiles(int k, int32_t* out, int cap) {
  int nt, ct;
  ck_tiles(k, &nt, &ct);
  for (int t = 0; t < nt && t < cap; ++t) ck_tile(k, t, &out[2 * t], &out[2 * t + 1]);
  return nt;
}

// 0, 1 (max_it iterations ran without a stop) or minus what ck_validate answered
int ck_host_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                  const double* val, const double* e, int64_t power_it, double alpha_frac, double tol, int64_t max_it, int chunk, double* u,
                  double* l_out, int64_t* T_out, double* err_hist, int64_t cap) {
  char msg[256];
  const int rc = ck_validate(n, M, row_ptr, col, W, k, m, ind, power_it, alpha_frac, max_it, msg, sizeof msg);
  if (rc) return -rc;
  return ck_host_reference(n, row_ptr, col, W, k, m, ind, val, e, power_it, alpha_frac, tol, max_it, chunk, u, l_out, T_out, err_hist, cap);
}
}

#ifdef CK_PLAN_MAIN
int main() {
  // 70 vertices (two partials) on a ring, vertex i joined to i +- 1 and i +- 17 with a weight that depends on the pair; vertex 5 stores no
  // entry, so the matrix is not symmetric there
  const int64_t n = 70;
  std::vector<int64_t> row_ptr(1, 0);
  std::vector<int32_t> col;
  std::vector<double> W;
  for (int64_t i = 0; i < n; ++i) {
    if (i != 5) {
      int32_t c[4] = {(int32_t)((i + 1) % n), (int32_t)((i + 17) % n), (int32_t)((i + n - 1) % n), (int32_t)((i + n - 17) % n)};
      for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
          if (c[b] < c[a]) { const int32_t t = c[a]; c[a] = c[b]; c[b] = t; }
      for (int a = 0; a < 4; ++a) { col.push_back(c[a]); W.push_back(0.25 + 0.01 * (double)((i + c[a]) % 13)); }
    }
    row_ptr.push_back((int64_t)col.size());
  }
  const int32_t ind[4] = {0, 17, 40, 69};
  const int k = 17;
  std::vector<double> val((size_t)4 * k, -0.25), e((size_t)n);
  for (int q = 0; q < 4; ++q) val[(size_t)q * k + q] = 0.75;
  for (int64_t i = 0; i < n; ++i) e[i] = 0.1 + 0.01 * (double)((i * 37) % 61);
  if (ck_host_validate(n, (int64_t)col.size(), row_ptr.data(), col.data(), W.data(), k, 4, ind, 100, 1.05, 1000)) return 1;
  int32_t tiles[64];
  if (ck_host_tiles(k, tiles, 32) != 2 || tiles[1] + tiles[3] != k) return 2;
  std::vector<double> u[3];
  double l[3], hist[3][1000];
  int64_t T[3];
  const int chunks[3] = {1, 7, 64};
  for (int q = 0; q < 3; ++q) {
    u[q].assign((size_t)n * k, 0.0);
    if (ck_host_solve(n, (int64_t)col.size(), row_ptr.data(), col.data(), W.data(), k, 4, ind, val.data(), e.data(), 100, 1.05, 1e-8, 1000,
                      chunks[q], u[q].data(), &l[q], &T[q], hist[q], 1000)) {
      printf("no stop: T %lld l %g\n", (long long)T[q], l[q]);
      return 3;
    }
    if (q && (T[q] != T[0] || memcmp(u[q].data(), u[0].data(), (size_t)n * k * 8) || memcmp(&l[q], &l[0], 8) ||
              memcmp(hist[q], hist[0], (size_t)T[0] * 8)))
      return 4;
  }
  printf("ok T %lld l %.17g u %g %g\n", (long long)T[0], l[0], u[0][0], u[0][(size_t)k * 30]);
  return 0;
}
#endif
