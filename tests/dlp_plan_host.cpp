// csrc/dlp_plan.h on the host, behind a C interface for tests/test_dlp_host.py (tests/dlp_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  With -DDLP_PLAN_MAIN it is a stand-alone program that walks a small graph
// through every function (for a host sanitizer run: g++ -fsanitize=address,undefined -DDLP_PLAN_MAIN).
#include "dlp_plan.h"
#include <cstring>

extern "C" {

int dlp_host_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m, const int32_t* ind,
                      double alpha, double lam, int64_t T) {
  char msg[256];
  return dlp_validate(n, M, row_ptr, col, P, k, m, ind, alpha, lam, T, msg, sizeof msg);
}

// the plan of valid arrays: tptr (n + 1), tcol (M), tval (M), lab (n), sizes[6] = partials, column tiles, widest tile, workspace values,
// sparse passes, Gram passes
void dlp_host_plan(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m, const int32_t* ind,
                   int64_t T, int64_t* tptr, int32_t* tcol, double* tval, int32_t* lab, int64_t* sizes) {
  DlpPlan plan;
  dlp_make_plan(n, M, row_ptr, col, P, k, m, ind, T, &plan);
  memcpy(tptr, plan.tptr.data(), (size_t)(n + 1) * sizeof(int64_t));
  if (M > 0) {
    memcpy(tcol, plan.tcol.data(), (size_t)M * sizeof(int32_t));
    memcpy(tval, plan.tval.data(), (size_t)M * sizeof(double));
  }
  memcpy(lab, plan.lab.data(), (size_t)n * sizeof(int32_t));
  sizes[0] = plan.P;
  sizes[1] = plan.ntiles;
  sizes[2] = plan.ct;
  sizes[3] = plan.work;
  sizes[4] = plan.sparse;
  sizes[5] = plan.grams;
}

// 0, or minus what dlp_validate answered; hist may be null
int dlp_host_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m, const int32_t* ind,
                   const double* val, double alpha, double lam, int64_t T, double* u, double* hist) {
  char msg[256];
  const int rc = dlp_validate(n, M, row_ptr, col, P, k, m, ind, alpha, lam, T, msg, sizeof msg);
  if (rc) return -rc;
  dlp_host_reference(n, M, row_ptr, col, P, k, m, ind, val, alpha, lam, T, u, hist);
  return 0;
}
}

#ifdef DLP_PLAN_MAIN
int main() {
  // 70 vertices (two partials): vertex i stores i + 1, i + 17, i - 1 (mod n) and, for even i, i - 17, with values that depend on the pair,
  // so the matrix is not symmetric; vertex 5 stores no entry
  const int64_t n = 70;
  std::vector<int64_t> row_ptr(1, 0);
  std::vector<int32_t> col;
  std::vector<double> P;
  for (int64_t i = 0; i < n; ++i) {
    if (i != 5) {
      int32_t c[4] = {(int32_t)((i + 1) % n), (int32_t)((i + 17) % n), (int32_t)((i + n - 1) % n), (int32_t)((i + n - 17) % n)};
      const int cnt = i % 2 == 0 ? 4 : 3;
      for (int a = 0; a < cnt; ++a)
        for (int b = a + 1; b < cnt; ++b)
          if (c[b] < c[a]) { const int32_t t = c[a]; c[a] = c[b]; c[b] = t; }
      for (int a = 0; a < cnt; ++a) { col.push_back(c[a]); P.push_back(0.2 + 0.01 * (double)((i + c[a]) % 13) - (a == 2 ? 0.3 : 0.0)); }
    }
    row_ptr.push_back((int64_t)col.size());
  }
  const int64_t M = (int64_t)col.size();
  const int32_t ind[5] = {0, 17, 40, 69, 17};          // vertex 17 twice: its last row counts
  const int k = 17, m = 5;
  const int64_t T = 4;
  std::vector<double> val((size_t)m * k, 0.0);
  for (int q = 0; q < m; ++q) val[(size_t)q * k + q] = 1.0;
  if (dlp_host_validate(n, M, row_ptr.data(), col.data(), P.data(), k, m, ind, 0.05, 0.1, T)) return 1;
  if (dlp_host_validate(n, M, row_ptr.data(), col.data(), P.data(), 65, m, ind, 0.05, 0.1, T) != 9) return 2;
  std::vector<int64_t> tptr((size_t)n + 1);
  std::vector<int32_t> tcol((size_t)M), lab((size_t)n);
  std::vector<double> tval((size_t)M);
  int64_t sizes[6];
  dlp_host_plan(n, M, row_ptr.data(), col.data(), P.data(), k, m, ind, T, tptr.data(), tcol.data(), tval.data(), lab.data(), sizes);
  if (tptr[n] != M || sizes[0] != 2 || sizes[1] != 2 || sizes[3] != (2 * T + 2) * n * k || sizes[4] != T * T + T - 2 || sizes[5] != 6) return 3;
  if (lab[17] != 4 || lab[0] != 0 || lab[1] != -1) return 4;
  for (int64_t j = 0; j < n; ++j)
    for (int64_t e = tptr[j]; e < tptr[j + 1]; ++e)
      if (e > tptr[j] && tcol[e - 1] >= tcol[e]) return 5;
  std::vector<double> u((size_t)n * k), hist((size_t)T * n * k), u2((size_t)n * k);
  if (dlp_host_solve(n, M, row_ptr.data(), col.data(), P.data(), k, m, ind, val.data(), 0.05, 0.1, T, u.data(), hist.data())) return 6;
  if (dlp_host_solve(n, M, row_ptr.data(), col.data(), P.data(), k, m, ind, val.data(), 0.05, 0.1, T, u2.data(), nullptr)) return 7;
  if (memcmp(u.data(), u2.data(), u.size() * 8) || memcmp(u.data(), hist.data() + (size_t)(T - 1) * n * k, u.size() * 8)) return 8;
  if (u[(size_t)17 * k + 4] != 1.0 || u[(size_t)17 * k + 1] != 0.0) return 9;
  printf("ok T %lld u %.17g %.17g\n", (long long)T, u[(size_t)k * 30], u[(size_t)k * 31 + 2]);
  return 0;
}
#endif
