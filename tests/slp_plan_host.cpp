// csrc/slp_plan.h on the host, behind a C interface for tests/test_slp_host.py (tests/slp_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  With -DSLP_PLAN_MAIN it is a stand-alone program that walks a small graph
// through every function (for a host sanitizer run: g++ -fsanitize=address,undefined -DSLP_PLAN_MAIN).
#include "slp_plan.h"
#include <cstring>

extern "C" {

int slp_host_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                      const double* gamma, int C, int64_t m, const int32_t* ind) {
  char msg[256];
  return slp_validate(n, M, row_ptr, col, W, lam, gamma, C, m, ind, msg, sizeof msg);
}

int slp_host_reverse(int64_t n, const int64_t* row_ptr, const int32_t* col, int32_t* rev) {
  slp_reverse_index(n, row_ptr, col, rev);
  return 0;
}

// out: (first column, columns, record width) per tile; returns the number of tiles (at most cap are written)
int slp_host_tiles(int C, int32_t* out, int cap) {
  const std::vector<SlpTile> t = slp_tiles(C);
  for (size_t q = 0; q < t.size() && (int)q < cap; ++q) {
    out[3 * q] = t[q].c0;
    out[3 * q + 1] = t[q].cols;
    out[3 * q + 2] = t[q].cpad;
  }
  return (int)t.size();
}

// the contract walked on the host: u (n, C) after T iterations; nonzero: what slp_validate answered
int slp_host_iterate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                     const double* gamma, int C, int64_t m, const int32_t* ind, const double* val, int64_t T, double* u) {
  char msg[256];
  const int rc = slp_validate(n, M, row_ptr, col, W, lam, gamma, C, m, ind, msg, sizeof msg);
  if (rc) return rc;
  std::vector<int32_t> rev((size_t)M);
  slp_reverse_index(n, row_ptr, col, rev.data());
  const std::vector<int32_t> lab = slp_label_rows(n, m, ind);
  slp_host_reference(n, M, row_ptr, col, W, lam, gamma, rev.data(), C, lab.data(), val, T, u);
  return 0;
}
}

#ifdef SLP_PLAN_MAIN
int main() {
  // a directed triangle with a diagonal entry and a two-way edge: rows 0: (0, 1), 1: (0, 2), 2: (0)
  const int64_t row_ptr[4] = {0, 2, 4, 5};
  const int32_t col[5] = {0, 1, 0, 2, 0};
  const double W[5] = {0.7, 0.5, 0.5, 0.25, 1.0}, lam[5] = {0.4, 0.5, 0.5, 0.6, 0.3}, gamma[3] = {1 / 1.2, 1 / 0.75, 1.0};
  const int32_t ind[2] = {0, 2};
  const double val[2 * 17] = {1.0};
  double u[3 * 17];
  int32_t rev[5], tiles[3 * 8];
  if (slp_host_validate(3, 5, row_ptr, col, W, lam, gamma, 17, 2, ind)) return 1;
  slp_host_reverse(3, row_ptr, col, rev);
  const int32_t want[5] = {0, 2, 1, -1, -1};
  if (memcmp(rev, want, sizeof want)) return 2;
  if (slp_host_tiles(17, tiles, 8) != 2 || tiles[1] + tiles[4] != 17) return 3;
  if (slp_host_iterate(3, 5, row_ptr, col, W, lam, gamma, 17, 2, ind, val, 25, u)) return 4;
  printf("ok %g %g %g\n", u[0], u[17], u[34]);
  return 0;
}
#endif
