// Host build of the HIP-free headers of the radius search for tests/test_epsball_host.py: the tree-order squared distance
// (sqdist_tree.h), numpy's row sum restated (npsum_exact.h) and the search plan (ball_plan.h).  Compile with -ffp-contract=off.
#include "../graphlearning_amd/csrc/ball_plan.h"
#include "../graphlearning_amd/csrc/npsum_exact.h"
#include "../graphlearning_amd/csrc/sqdist_tree.h"

// out[r] = the distance between rows r of U and V (m rows of d coordinates)
extern "C" void eb_npsum_rows(const double* U, const double* V, int64_t m, int d, double* out) {
  for (int64_t r = 0; r < m; ++r) out[r] = npsum_sqdiff(U + r * d, V + r * d, d);
}
extern "C" void eb_sqdist_rows(const double* U, const double* V, int64_t m, int d, double* out) {
  for (int64_t r = 0; r < m; ++r) out[r] = sqdist_exact(U + r * d, V + r * d, d);
}

// iout: g, axis[3], nc[3], stride[3], ncells, coarsened, nqb (13 values); dout: lo[3], h[3]
extern "C" void eb_plan(int64_t n, int d, double epsilon, const double* lo, const double* hi, int64_t* iout, double* dout) {
  const BallPlan p = ball_make_plan(n, d, epsilon, lo, hi);
  int k = 0;
  iout[k++] = p.g;
  for (int a = 0; a < 3; ++a) iout[k++] = p.axis[a];
  for (int a = 0; a < 3; ++a) iout[k++] = p.nc[a];
  for (int a = 0; a < 3; ++a) iout[k++] = p.stride[a];
  iout[k++] = p.ncells;
  iout[k++] = p.coarsened;
  iout[k++] = p.nqb;
  for (int a = 0; a < 3; ++a) dout[a] = p.lo[a];
  for (int a = 0; a < 3; ++a) dout[3 + a] = p.h[a];
}

// the cell coordinates of m values on grid axis a of that plan
extern "C" void eb_cell_coords(int64_t n, int d, double epsilon, const double* lo, const double* hi, int a, const double* x, int64_t m,
                               int64_t* out) {
  const BallPlan p = ball_make_plan(n, d, epsilon, lo, hi);
  for (int64_t i = 0; i < m; ++i) out[i] = ball_cell_coord(p, a, x[i]);
}
