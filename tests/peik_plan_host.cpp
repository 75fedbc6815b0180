// csrc/peik_plan.h on the host, behind a C interface for tests/test_peikonal_host.py and the golden maker (tests/peik_ref.py:
// build_host_lib): g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  With -DPEIK_PLAN_MAIN it is a stand-alone program that walks
// small graphs through every function (for a host sanitizer run: g++ -fsanitize=address,undefined -DPEIK_PLAN_MAIN).
#include "../graphlearning_amd/csrc/peik_plan.h"
#include <cstring>

extern "C" {

int peik_host_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                       const int64_t* bptr, const int32_t* bidx, const double* bval, double p, int nbis, const double* u0) {
  char msg[256];
  return peik_validate(n, M, row_ptr, nbr, W, f, B, bptr, bidx, bval, p, nbis, u0, msg, sizeof msg);
}

// 0, minus what peik_validate answered, or PEIK_ECAP when the rounds pass their cap
int peik_host_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                    const int64_t* bptr, const int32_t* bidx, const double* bval, double p, int nbis, const double* u0, int64_t max_rounds,
                    double* u, int64_t* rounds_out) {
  char msg[256];
  const int rc = peik_validate(n, M, row_ptr, nbr, W, f, B, bptr, bidx, bval, p, nbis, u0, msg, sizeof msg);
  if (rc) return -rc;
  return peik_host_reference(n, row_ptr, nbr, W, f, B, bptr, bidx, bval, p, nbis, u0, max_rounds, u, rounds_out);
}

void peik_host_constants(int64_t* out) {
  out[0] = PEIK_MAX_COLS;
  out[1] = PEIK_MAX_BISECTION;
  out[2] = PEIK_MAX_VALUES;
  out[3] = PEIK_ECAP;
  out[4] = peik_round_cap(100, 1.0, 30);
  out[5] = peik_round_cap(100, 2.0, 30);
}
}

#ifdef PEIK_PLAN_MAIN
int main() {
  // the unit path of 7 vertices, both ends on the boundary at 0, f = 1, p = 1: u = 0 1 2 2.5 2 1 0
  // (the middle vertex solves (1 + 2 + 2) / 2 from its two neighbours at 2)
  const int64_t n = 7;
  std::vector<int64_t> row_ptr(1, 0);
  std::vector<int32_t> nbr;
  std::vector<double> W;
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0) { nbr.push_back((int32_t)(i - 1)); W.push_back(1.0); }
    if (i == 3) { nbr.push_back(3); W.push_back(5.0); }          // a stored self loop: skipped
    if (i + 1 < n) { nbr.push_back((int32_t)(i + 1)); W.push_back(1.0); }
    row_ptr.push_back((int64_t)nbr.size());
  }
  const int64_t M = (int64_t)nbr.size();
  std::vector<double> f((size_t)n, 1.0), u0((size_t)n, -7.0);
  const int64_t bptr[3] = {0, 2, 5};
  const int32_t bidx[5] = {0, 6, 0, 3, 0};                         // problem 1 lists vertex 0 twice: its last value counts
  const double bval[5] = {0.0, 0.0, 9.0, 0.5, 1.0};
  if (peik_host_validate(n, M, row_ptr.data(), nbr.data(), W.data(), f.data(), 2, bptr, bidx, bval, 1.0, 30, u0.data())) return 1;
  if (peik_host_validate(n, M, row_ptr.data(), nbr.data(), W.data(), f.data(), 257, bptr, bidx, bval, 1.0, 30, u0.data()) != 9) return 2;
  std::vector<double> u((size_t)n * 2), v((size_t)n * 2);
  int64_t rounds = 0;
  if (peik_host_solve(n, M, row_ptr.data(), nbr.data(), W.data(), f.data(), 2, bptr, bidx, bval, 1.0, 30, u0.data(), 0, u.data(), &rounds))
    return 3;
  const double want0[7] = {0, 1, 2, 2.5, 2, 1, 0};
  // from 1 at vertex 0 and 0.5 at vertex 3: vertex 1 solves (1 + 1 + 1.5) / 2 from both neighbours, vertex 2 (1 + 0.5) / 1 from vertex 3
  const double want1[7] = {1, 1.75, 1.5, 0.5, 1.5, 2.5, 3.5};
  for (int64_t i = 0; i < n; ++i)
    if (u[(size_t)i * 2] != want0[i] || u[(size_t)i * 2 + 1] != want1[i]) return 4;
  if (peik_host_solve(n, M, row_ptr.data(), nbr.data(), W.data(), f.data(), 2, bptr, bidx, bval, 1.0, 30, u0.data(), 2, v.data(), &rounds) !=
      PEIK_ECAP || rounds != 2)
    return 5;
  // p = 2 on the same path: u_1 solves (t - 0)^2 = 1 from the end alone, t = 1, to the resolution of 60 halvings
  if (peik_host_solve(n, M, row_ptr.data(), nbr.data(), W.data(), f.data(), 2, bptr, bidx, bval, 2.0, 60, u0.data(), 0, v.data(), &rounds))
    return 6;
  if (std::fabs(v[2] - 1.0) > 1e-14) return 7;
  // a second component nobody reaches takes u0: vertices 7 and 8 joined to each other only
  std::vector<int64_t> rp2(row_ptr);
  std::vector<int32_t> nb2(nbr);
  std::vector<double> W2(W), f2((size_t)n + 2, 1.0), u02((size_t)n + 2, -7.0);
  nb2.push_back(8); W2.push_back(1.0); rp2.push_back((int64_t)nb2.size());
  nb2.push_back(7); W2.push_back(1.0); rp2.push_back((int64_t)nb2.size());
  std::vector<double> w((size_t)(n + 2) * 2);
  if (peik_host_solve(n + 2, (int64_t)nb2.size(), rp2.data(), nb2.data(), W2.data(), f2.data(), 2, bptr, bidx, bval, 1.0, 30, u02.data(), 0,
                      w.data(), &rounds))
    return 8;
  if (w[(size_t)7 * 2] != -7.0 || w[(size_t)8 * 2 + 1] != -7.0 || w[(size_t)3 * 2] != 2.5) return 9;
  printf("ok rounds %lld u %.17g %.17g\n", (long long)rounds, u[6], v[6]);
  return 0;
}
#endif
