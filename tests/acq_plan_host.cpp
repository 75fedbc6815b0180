// csrc/acq_plan.h on the host, behind a C interface for tests/test_al_host.py (tests/al_ref.py: build_host_lib):
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.  With -DACQ_PLAN_MAIN it is a stand-alone program that walks a small problem
// through every function (for a host sanitizer run: g++ -fsanitize=address,undefined -DACQ_PLAN_MAIN).
#include "acq_plan.h"
#include <cstring>

extern "C" {

int acq_host_validate_state(int64_t n, int M, const double* V, const double* C, double gamma2) {
  char msg[256];
  return acq_validate_state(n, M, V, C, gamma2, msg, sizeof msg);
}

int acq_host_validate_cand(int64_t n, int kind, int greedy, const int32_t* cand, int64_t nc) {
  char msg[256];
  return acq_validate_cand(n, kind, greedy != 0, cand, nc, msg, sizeof msg);
}

// out[0] candidates per workgroup of the pass, [1] its bytes of LDS, [2] bytes of LDS of the update (0: C stays in L2)
void acq_host_tiling(int M, int64_t* out) {
  out[0] = acq_tile_rows(M);
  out[1] = (int64_t)acq_pass_lds_bytes(M);
  out[2] = (int64_t)acq_update_lds_bytes(M);
}

// 0, or minus what the validation answered
int acq_host_compute_c(int64_t n, int M, const double* V, const double* C, double gamma2, int kind, const int32_t* cand, int64_t nc,
                       const double* unc, double* vals) {
  char msg[256];
  int rc = acq_validate_state(n, M, V, C, gamma2, msg, sizeof msg);
  if (!rc) rc = acq_validate_cand(n, kind, false, cand, nc, msg, sizeof msg);
  if (!rc && !unc && kind >= ACQ_MC) rc = 3;
  if (rc) return -rc;
  acq_host_compute(n, M, V, C, gamma2, kind, cand, nc, unc, vals);
  return 0;
}

// C is updated in place
int acq_host_update_c(int64_t n, int M, const double* V, double* C, double gamma2, const int32_t* query, int64_t nq) {
  char msg[256];
  const int rc = acq_validate_cand(n, ACQ_VAR, false, query, nq, msg, sizeof msg);
  if (rc) return -rc;
  acq_host_update(M, V, C, gamma2, query, nq);
  return 0;
}

// 0; -100: more rounds than distinct vertices; r + 1: round r had no finite maximum; minus a validation code otherwise
int64_t acq_host_greedy_c(int64_t n, int M, const double* V, const double* C, double gamma2, int kind, const int32_t* cand, int64_t nc, int64_t b,
                          int32_t* queries, double* vals) {
  char msg[256];
  const int rc = acq_validate_cand(n, kind, true, cand, nc, msg, sizeof msg);
  if (rc) return -rc;
  const int64_t out = acq_host_greedy(n, M, V, C, gamma2, kind, cand, nc, b, queries, vals);
  return out == -1 ? -100 : out;
}

int acq_host_better(double val, int32_t pos, double bval, int32_t bpos) { return acq_better(val, pos, bval, bpos) ? 1 : 0; }
}

#ifdef ACQ_PLAN_MAIN
int main() {
  // 70 vertices (two tiles of the pass, the second short), 5 columns; vertex 69 repeats vertex 3
  const int64_t n = 70;
  const int M = 5;
  std::vector<double> V((size_t)n * M), C((size_t)M * M, 0.0), C2, vals((size_t)n), unc((size_t)n, 0.5);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < M; ++j) V[i * M + j] = 0.01 * (double)(((i + 3) * (j + 2) * 31) % 41) - 0.2;
  for (int j = 0; j < M; ++j) {
    V[69 * M + j] = V[3 * M + j];
    C[j * M + j] = 1.0 / (0.1 * j + 0.01);
  }
  if (acq_host_validate_state(n, M, V.data(), C.data(), 0.01)) return 1;
  if (acq_host_validate_state(n, 257, V.data(), C.data(), 0.01) != 8) return 2;
  std::vector<int32_t> cand((size_t)n);
  for (int64_t i = 0; i < n; ++i) cand[i] = (int32_t)(n - 1 - i);          // unsorted; position 0 is vertex 69, position 66 vertex 3
  for (int kind = 0; kind < 4; ++kind)
    if (acq_host_compute_c(n, M, V.data(), C.data(), 0.01, kind, cand.data(), n, unc.data(), vals.data())) return 3;
  if (acq_host_compute_c(n, M, V.data(), C.data(), 0.01, ACQ_VAR, cand.data(), n, nullptr, vals.data())) return 3;
  if (vals[0] != vals[66]) return 4;
  int32_t q[3];
  double qv[3];
  if (acq_host_greedy_c(n, M, V.data(), C.data(), 0.01, ACQ_VAR, cand.data(), n, 3, q, qv)) return 5;
  C2 = C;
  const int32_t first = cand[q[0]];
  if (acq_host_update_c(n, M, V.data(), C2.data(), 0.01, &first, 1)) return 6;
  if (acq_host_compute_c(n, M, V.data(), C2.data(), 0.01, ACQ_VAR, cand.data(), n, nullptr, vals.data())) return 6;
  if (vals[q[1]] != qv[1]) return 7;
  cand[1] = cand[0];          // 70 positions, 69 distinct vertices: refused before a round runs
  if (acq_host_greedy_c(n, M, V.data(), C.data(), 0.01, ACQ_VAR, cand.data(), n, n, q, qv) != -100) return 8;
  if (acq_host_validate_cand(n, ACQ_MC, 1, cand.data(), n) != 3) return 9;
  int64_t tile[3];
  acq_host_tiling(256, tile);
  if (tile[0] != 8 || tile[1] != 2 * 8 * 257 * 8 || tile[2] != 0) return 10;
  printf("ok first %d value %.17g\n", first, qv[0]);
  return 0;
}
#endif
