// csrc/eig_plan.h on the host, behind a C interface for tests/test_eig_host.py (tests/eig_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  The calls mirror glx_eig_* one for one with loops standing in for the kernels;
// a call answers 0, or minus what eig_validate said, or the number of the argument that is out of range.  With -DEIG_PLAN_MAIN it is
// a stand-alone program that walks a small graph through every operation (for a host sanitizer run:
// g++ -fsanitize=address,undefined -DEIG_PLAN_MAIN).
#include "eig_plan.h"

extern "C" {

int eig_host_validate(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int64_t m) {
  char msg[256];
  return eig_validate(n, row_ptr, col, val, m, msg, sizeof msg);
}

int64_t eig_host_basis_size(int64_t n, int64_t k) { return eig_basis_size(n, k); }
int64_t eig_host_device_bytes(int64_t n, int64_t nnz, int64_t m) { return eig_device_bytes(n, nnz, m); }

int eig_host_create(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int m, EigHost** out) {
  char msg[256];
  const int rc = eig_validate(n, row_ptr, col, val, m, msg, sizeof msg);
  if (rc) return -rc;
  *out = new EigHost;
  (*out)->create(n, row_ptr, col, val, m);
  return 0;
}
int eig_host_set_column(EigHost* e, int j, const double* x) { return e->set_column(j, x); }
int eig_host_orthonormalize(EigHost* e, int j, double* norm) { return e->orthonormalize(j, norm); }
int eig_host_run(EigHost* e, int j0, int j1, double* alpha, double* beta) { return e->run(j0, j1, alpha, beta); }
int eig_host_rotate(EigHost* e, const double* Y, int rows, int keep) { return e->rotate(Y, rows, keep); }
int eig_host_get_columns(EigHost* e, int j0, int j1, double* out) { return e->get_columns(j0, j1, out); }
void eig_host_destroy(EigHost* e) { delete e; }
}

#ifdef EIG_PLAN_MAIN
int main() {
  // 70 vertices (two partials) on a ring, vertex i joined to i +- 1 and i +- 17 with a weight that depends on the pair, plus a diagonal
  const int64_t n = 70;
  std::vector<int64_t> row_ptr(1, 0);
  std::vector<int32_t> col;
  std::vector<double> val;
  for (int64_t i = 0; i < n; ++i) {
    int32_t c[5] = {(int32_t)i, (int32_t)((i + 1) % n), (int32_t)((i + 17) % n), (int32_t)((i + n - 1) % n), (int32_t)((i + n - 17) % n)};
    for (int a = 0; a < 5; ++a)
      for (int b = a + 1; b < 5; ++b)
        if (c[b] < c[a]) { const int32_t t = c[a]; c[a] = c[b]; c[b] = t; }
    for (int a = 0; a < 5; ++a) { col.push_back(c[a]); val.push_back(c[a] == i ? 1.5 : 0.25 + 0.01 * (double)((i + c[a]) % 13)); }
    row_ptr.push_back((int64_t)col.size());
  }
  const int m = 20;
  if (eig_host_basis_size(n, 5) != m || eig_host_device_bytes(n, (int64_t)col.size(), m) <= 0) return 1;
  EigHost* e = nullptr;
  if (eig_host_create(n, row_ptr.data(), col.data(), val.data(), m, &e)) return 2;
  std::vector<double> x((size_t)n), alpha((size_t)m), beta((size_t)m), Y((size_t)m * 12, 0.0), out((size_t)(m + 1) * n);
  for (int64_t i = 0; i < n; ++i) x[i] = 0.1 + 0.01 * (double)((i * 37) % 61);
  double norm = 0.0;
  if (eig_host_set_column(e, 0, x.data()) || eig_host_orthonormalize(e, 0, &norm) || !(norm > 0.0)) return 3;
  if (eig_host_run(e, 0, m, alpha.data(), beta.data())) return 4;
  for (int q = 0; q < 12; ++q) Y[(size_t)q * 12 + q] = 1.0;          // keeps the first twelve columns as they are
  if (eig_host_rotate(e, Y.data(), m, 12) || eig_host_run(e, 12, m, alpha.data(), beta.data())) return 5;
  if (eig_host_set_column(e, m, x.data()) || eig_host_orthonormalize(e, m, &norm)) return 6;
  if (eig_host_get_columns(e, 0, m + 1, out.data())) return 7;
  if (eig_host_run(e, 3, 3, alpha.data(), beta.data()) != 2 || eig_host_rotate(e, Y.data(), m + 1, 1) != 3 || eig_host_set_column(e, m + 1, x.data()) != 2)
    return 8;
  printf("ok alpha %.17g beta %.17g norm %.3g v %g\n", alpha[0], beta[0], norm, out[(size_t)3 * n + 5]);
  eig_host_destroy(e);
  return 0;
}
#endif
