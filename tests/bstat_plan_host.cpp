// Stand-alone host program for csrc/bstat_plan.h and the term walk of csrc/npsum_exact.h (tests/test_boundary_host.py builds and
// runs it; it may be built with -fsanitize=address,undefined).  It runs the header's arithmetic on plain memory: the test writes the
// inputs into a file, the program writes the results into another, the test compares them bit for bit with tests/boundary_ref.py and
// with numpy.
//
//   bstat_plan_host stat IN OUT
//     IN:  int64 n, d, nnz, k, flags, wave_row; double X[n * d]; int32 indptr[n + 1]; int32 indices[nnz]; int32 J[n * k]
//     OUT: int64 status (0; 1 + the first vertex without a normal; -1: the arguments were refused, the reason on stdout),
//          int64 rows[3] (short class, wavefront class, full rows); double T[n]; double nu[n * d]
//   bstat_plan_host npsum IN OUT
//     IN:  int64 rows, d; double U[rows * d], V[rows * d], W[rows * d]
//     OUT: double [4][rows]: np.sum((U - V)^2), np.sum(U * V), np.sum((U - V) * W), np.sum((U - V) * ((W + U) / 2)) per row
#include "bstat_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
template <class T>
bool get(FILE* f, std::vector<T>* v, size_t count) {
  v->resize(count);
  return count == 0 || fread(v->data(), sizeof(T), count, f) == count;
}
template <class T>
bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int run_stat(FILE* in, FILE* out) {
  std::vector<int64_t> h;
  if (!get(in, &h, 6)) return 2;
  const int64_t n = h[0], nnz = h[2];
  const int d = (int)h[1], k = (int)h[3], flags = (int)h[4], wave_row = (int)h[5];
  if (n < 1 || n > (1 << 24) || d < 1 || d > (1 << 16) || nnz < 0 || nnz > (1 << 28) || k < 0 || k > (1 << 16)) return 2;
  std::vector<double> X;
  std::vector<int32_t> indptr, indices, J;
  if (!get(in, &X, (size_t)n * d) || !get(in, &indptr, (size_t)n + 1) || !get(in, &indices, (size_t)nnz) || !get(in, &J, (size_t)n * k))
    return 2;
  std::vector<int64_t> head(4, 0);
  std::vector<double> T((size_t)n, 0.0), nu((size_t)n * d, 0.0);
  char why[200];
  int64_t maxdeg = 0;
  if (bstat_check(n, d, indptr.data(), indices.data(), nnz, k, k ? J.data() : nullptr, &maxdeg, why, sizeof why)) {
    printf("refused: %s\n", why);
    head[0] = -1;
  } else {
    head[0] = bstat_host(n, d, X.data(), indptr.data(), indices.data(), k, k ? J.data() : nullptr, flags, T.data(), nu.data(), wave_row,
                         head.data() + 1);
    printf("n=%lld d=%d nnz=%lld k=%d flags=%d maxdeg=%lld status=%lld\n", (long long)n, d, (long long)nnz, k, flags, (long long)maxdeg,
           (long long)head[0]);
  }
  return put(out, head) && put(out, T) && put(out, nu) ? 0 : 2;
}

int run_npsum(FILE* in, FILE* out) {
  std::vector<int64_t> h;
  if (!get(in, &h, 2)) return 2;
  const int64_t rows = h[0];
  const int d = (int)h[1];
  if (rows < 1 || rows > (1 << 20) || d < 1 || d > (1 << 20)) return 2;
  std::vector<double> U, V, W;
  if (!get(in, &U, (size_t)rows * d) || !get(in, &V, (size_t)rows * d) || !get(in, &W, (size_t)rows * d)) return 2;
  std::vector<double> res((size_t)4 * rows);
  for (int64_t r = 0; r < rows; ++r) {
    const double *u = U.data() + (size_t)r * d, *v = V.data() + (size_t)r * d, *w = W.data() + (size_t)r * d;
    res[r] = npsum_sqdiff(u, v, d);
    res[rows + r] = npsum_dot(u, v, d);
    res[2 * rows + r] = npsum_terms(BstatTerm{u, v, w, nullptr}, d);
    res[3 * rows + r] = npsum_terms(BstatTerm{u, v, w, u}, d);
  }
  return put(out, res) ? 0 : 2;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "stat") && strcmp(argv[1], "npsum"))) {
    fprintf(stderr, "usage: bstat_plan_host stat|npsum IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  int rc = 2;
  if (in && out) rc = strcmp(argv[1], "stat") ? run_npsum(in, out) : run_stat(in, out);
  if (in) fclose(in);
  if (out) fclose(out);
  if (rc) fprintf(stderr, "bstat_plan_host: bad input\n");
  else printf("bstat_plan_host: ok\n");
  return rc;
}
