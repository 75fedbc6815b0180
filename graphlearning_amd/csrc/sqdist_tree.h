// Squared Euclidean distance with the accumulation order of scipy's cKDTree (sqeuclidean_distance_double): four partial sums over
// blocks of four coordinates, combined left to right, then the remaining coordinates one by one; no fused multiply-add.  The
// exact kNN search (knn_rerank.hip) ranks by it and the radius search (ball.hip) decides membership by it, so that both agree with
// the tree of the reference bit for bit.  No HIP header: tests/epsball_host.cpp compiles it for the host.
#pragma once

#if defined(__HIPCC__)
#define SQDIST_FN __host__ __device__ __forceinline__
#else
#define SQDIST_FN static inline
#endif

SQDIST_FN double sqdist_exact(const double* __restrict__ u, const double* __restrict__ v, int d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  int i = 0;
  for (; i + 4 <= d; i += 4) {
    const double d0 = u[i] - v[i], d1 = u[i + 1] - v[i + 1], d2 = u[i + 2] - v[i + 2], d3 = u[i + 3] - v[i + 3];
    a0 = a0 + d0 * d0;
    a1 = a1 + d1 * d1;
    a2 = a2 + d2 * d2;
    a3 = a3 + d3 * d3;
  }
  double s = a0 + a1 + a2 + a3;
  for (; i < d; ++i) {
    const double dd = u[i] - v[i];
    s = s + dd * dd;
  }
  return s;
}
