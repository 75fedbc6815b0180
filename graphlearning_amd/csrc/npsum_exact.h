// numpy's sum over one contiguous row, restated: `np.sum(V * V, axis=1)` with V = x_i - x_j is what the reference's epsilon-ball
// weights see (graphlearning/weightmatrix.py:245-246), and its bits depend on numpy's pairwise summation:
//   fewer than 8 terms    the plain left-to-right sum;
//   8 .. 128 terms        eight accumulators r[j] = t[j], r[j] += t[i + j] for i = 8, 16, ... below n - n % 8, combined as
//                         ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining terms one by one;
//   more than 128 terms   split at n2 = n / 2 rounded down to a multiple of 8, left part + right part, each by the same rule.
// The walk is written once over a term functor t(i) (npsum_terms): the squared difference t[i] = fl(fl(u[i] - v[i])^2) of the
// epsilon-ball weights (npsum_sqdiff), the product of two rows (npsum_dot), and whatever another caller rounds per term (the
// boundary statistic's (x_i - x_j) * nu2, bstat_plan.h).  A functor rounds every operation of its term on its own: no fused
// multiply-add inside it either.  For fewer than 8 coordinates npsum_sqdiff is the same expression as sqdist_exact (sqdist_tree.h);
// from 8 on the two differ.  No HIP header: tests/epsball_host.cpp and tests/bstat_plan_host.cpp compile it for the host and
// tests/test_epsball_host.py, tests/test_boundary_host.py compare it with numpy for every row length from 1 to 300.
#pragma once

#if defined(__HIPCC__)
#define NPSUM_FN __host__ __device__ inline
#define NPSUM_FN_MEMBER __host__ __device__ inline
#else
#define NPSUM_FN static inline
#define NPSUM_FN_MEMBER inline
#endif

// rows of at most 128 terms: terms off .. off + n - 1 of the row
template <class Term>
NPSUM_FN double npsum_terms_leaf(const Term& t, int off, int n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const double ti = t(off + i);
      s = s + ti;
    }
    return s;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = t(off + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    for (int j = 0; j < 8; ++j) {
      const double ti = t(off + i + j);
      r[j] = r[j] + ti;
    }
  }
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) {
    const double ti = t(off + i);
    s = s + ti;
  }
  return s;
}

// np.sum over the d terms t(0) .. t(d - 1).  The recursion above 128 terms is walked with an explicit stack (a part is at least
// half of its parent minus 7 terms, so 32 levels serve any int d).
template <class Term>
NPSUM_FN double npsum_terms(const Term& t, int d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (d <= 128) return npsum_terms_leaf(t, 0, d);
  int s_off[32], s_n[32], s_stage[32];
  double s_left[32];
  int sp = 0;
  s_off[0] = 0;
  s_n[0] = d;
  s_stage[0] = 0;
  double ret = 0.0;
  while (sp >= 0) {
    const int off = s_off[sp], n = s_n[sp];
    if (n <= 128) {
      ret = npsum_terms_leaf(t, off, n);
      --sp;
      continue;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    if (s_stage[sp] == 0) {
      s_stage[sp] = 1;
      ++sp;
      s_off[sp] = off;
      s_n[sp] = n2;
      s_stage[sp] = 0;
    } else if (s_stage[sp] == 1) {
      s_left[sp] = ret;
      s_stage[sp] = 2;
      ++sp;
      s_off[sp] = off + n2;
      s_n[sp] = n - n2;
      s_stage[sp] = 0;
    } else {
      ret = s_left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

// t[i] = fl(fl(u[i] - v[i])^2)
struct NpsumSqdiff {
  const double* __restrict__ u;
  const double* __restrict__ v;
  NPSUM_FN_MEMBER double operator()(int i) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dd = u[i] - v[i];
    return dd * dd;
  }
};

// t[i] = fl(u[i] * v[i])
struct NpsumProduct {
  const double* __restrict__ u;
  const double* __restrict__ v;
  NPSUM_FN_MEMBER double operator()(int i) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return u[i] * v[i];
  }
};

// np.sum((u - v) * (u - v)) over d coordinates
NPSUM_FN double npsum_sqdiff(const double* __restrict__ u, const double* __restrict__ v, int d) { return npsum_terms(NpsumSqdiff{u, v}, d); }
// np.sum(u * v) over d coordinates
NPSUM_FN double npsum_dot(const double* __restrict__ u, const double* __restrict__ v, int d) { return npsum_terms(NpsumProduct{u, v}, d); }
