// Host build of the level plan of the in-order Gauss-Seidel sweeps (lip_plan.h) for tests/test_amle_host.py, and a host restatement
// of the sweeps in two forms -- vertex after vertex in index order, and level after level of that plan with every level walked
// BACKWARDS (within a level the order must not matter) -- for the cases that are too long for the Python forms of tests/amle_ref.py.
// Compile with -ffp-contract=off.
#include "../graphlearning_amd/csrc/lip_plan.h"

extern "C" void lph_constants(int64_t* out) {
  out[0] = LIP_SMALL;
  out[1] = LIP_BLOCK;
  out[2] = LIP_CHUNK;
}

// level_out (n), order_out (n), lvl_ptr_out (n + 1), launches_out (3 * n: lvl0, lvl1, merged); counts_out: levels, ordered vertices, launches
extern "C" void lph_plan(int64_t n, const int64_t* row_ptr, const int32_t* nbr, const unsigned char* bdy, int small, int32_t* level_out,
                         int32_t* order_out, int64_t* lvl_ptr_out, int32_t* launches_out, int64_t* counts_out) {
  const LipPlan p = lip_make_plan(n, row_ptr, nbr, bdy, small);
  for (int64_t i = 0; i < n; ++i) level_out[i] = p.level[i];
  for (size_t q = 0; q < p.order.size(); ++q) order_out[q] = p.order[q];
  for (size_t q = 0; q < p.lvl_ptr.size(); ++q) lvl_ptr_out[q] = p.lvl_ptr[q];
  for (size_t q = 0; q < p.launches.size(); ++q) {
    launches_out[3 * q] = p.launches[q].lvl0;
    launches_out[3 * q + 1] = p.launches[q].lvl1;
    launches_out[3 * q + 2] = p.launches[q].merged;
  }
  counts_out[0] = p.nlevels;
  counts_out[1] = (int64_t)p.order.size();
  counts_out[2] = (int64_t)p.launches.size();
}

#define LMIN(a, b) (((a) < (b)) ? (a) : (b))
#define LMAX(a, b) (((a) > (b)) ? (a) : (b))
#define LABS(a) (((a) < 0) ? -(a) : (a))

static double lph_value(const double* u, const int32_t* nbr, const double* W, int64_t e0, int64_t e1, int weighted, double alpha,
                        double beta) {
  double minu = u[nbr[e0]], maxu = u[nbr[e0]];
  if (!weighted) {
    double sumu = 0.0, deg = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
      sumu += W[e] * u[nbr[e]];
      deg += W[e];
      minu = LMIN(u[nbr[e]], minu);
      maxu = LMAX(u[nbr[e]], maxu);
    }
    return alpha * sumu / deg + beta * (minu + maxu) / 2;
  }
  for (int64_t e = e0; e < e1; ++e) {
    minu = LMIN(u[nbr[e]], minu);
    maxu = LMAX(u[nbr[e]], maxu);
  }
  double a = minu, b = maxu;
  for (int k = 0; k < 30; ++k) {
    double minw = 0, maxw = 0;
    const double t = (a + b) / 2.0;
    for (int64_t e = e0; e < e1; ++e) {
      minw = LMIN(W[e] * (t - u[nbr[e]]), minw);
      maxw = LMAX(W[e] * (t - u[nbr[e]]), maxw);
    }
    if (minw + maxw > 0) b = t; else a = t;
  }
  return (a + b) / 2.0;
}

// u (n): zeros with the boundary values set, updated in place.  levelled != 0: by the plan's levels, each walked backwards.
// errs (T) or null.  Returns the sweeps done.
extern "C" int64_t lph_sweeps(int64_t n, const int64_t* row_ptr, const int32_t* nbr, const double* W, const unsigned char* bdy, double* u,
                              int weighted, double alpha, double beta, int64_t T, double tol, int levelled, double* errs) {
  std::vector<int32_t> visit;
  if (levelled) {
    const LipPlan p = lip_make_plan(n, row_ptr, nbr, bdy);
    for (int64_t l = 0; l < p.nlevels; ++l)
      for (int64_t q = p.lvl_ptr[l + 1] - 1; q >= p.lvl_ptr[l]; --q) visit.push_back(p.order[q]);
  } else {
    for (int64_t i = 0; i < n; ++i)
      if (!bdy[i]) visit.push_back((int32_t)i);
  }
  int64_t it = 0;
  for (; it < T; ++it) {
    double err = 0;
    for (const int32_t i : visit) {
      const double ne = lph_value(u, nbr, W, row_ptr[i], row_ptr[i + 1], weighted, alpha, beta);
      err = LMAX(LABS(u[i] - ne), err);
      u[i] = ne;
    }
    if (errs) errs[it] = err;
    if (err < tol && it > 20) return it + 1;
  }
  return it;
}
