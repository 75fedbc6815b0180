// The plan of one radius search (ball.hip): everything it derives on the host from (n, d, epsilon) and the bounding box of the
// points before it touches the device -- the axes of the cell grid, the cell side and the cells per axis, the caps -- and the
// constants it shares with the kernels.  No HIP header: tests/test_epsball_host.py builds it on the host (tests/epsball_host.cpp)
// and checks the plans of a table of shapes.
//
// The grid is a FILTER: membership is decided by the exact test alone (sqdist_exact(x, y) <= fl(epsilon * epsilon)), the cells
// only say which pairs need not be tested.  A point's cell coordinate on a grid axis is c = floor(fl(fl(x - lo) / h)), clamped
// to [0, nc - 1].  Two points whose coordinates differ by two or more on one axis are skipped, which is safe because
//   * the computed quotient is within 3 * 2^-53 relative of the true one and is below 2^20 (BALL_AXIS_CAP), so a difference of
//     more than 1 between two computed quotients means the true |x - y| exceeds h (1 - 2^-30);
//   * h >= epsilon (1 + 1e-6), so |x - y| > epsilon (1 + 9e-7), the single term fl(fl(x - y)^2) already exceeds fl(epsilon^2),
//     and a sum of non-negative terms is monotone in floating point: the exact test would have refused the pair;
//   * h >= 1e-150, so the argument survives epsilon = 0 and an epsilon whose square underflows: the term is at least 9e-301 > 0.
// Clamping merges cells at the upper end of an axis, and coarsening (below) multiplies h: cells only ever grow.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

static const int BALL_BQ = 64;                     // sorted queries per workgroup of the count / fill kernels: one wavefront, one query per lane
static const int BALL_TILE = 64;                   // candidate rows staged in LDS at a time (one per lane)
static const int BALL_REG_D = 3;                   // up to this many coordinates the query stays in registers and the tile in LDS
static const int BALL_SORT_CAP = 2048;             // longest row one wavefront sorts in LDS (8 KB); longer rows ("hubs") get a workgroup each
static const int BALL_GRID_AXES = 3;               // grid axes at most
static const int64_t BALL_AXIS_CAP = 1 << 20;      // cells per axis at most (see above)
static const int64_t BALL_CELL_CAP = 1 << 21;      // cells in all at most (and at most 4 per point, 1024 allowed): beyond it every axis is coarsened
static const double BALL_H_MARGIN = 1.0 + 1e-6;    // cell side / epsilon at least
static const double BALL_H_MIN = 1e-150;           // cell side at least
static const int64_t BALL_NNZ_MAX = 2147483647;    // entries of a CSR matrix with int32 row pointers

struct BallPlan {
  int g;                  // grid axes in use (>= 1; an axis may have a single cell)
  int axis[3];            // the coordinate behind grid axis a; the LAST axis runs fastest in the cell id
  double lo[3], h[3];     // lower end of the box and cell side per grid axis
  int64_t nc[3];          // cells per grid axis
  int64_t ncells;         // product
  int64_t stride[3];      // cell id = sum c[a] * stride[a]
  int coarsened;          // times the cell sides were multiplied to respect BALL_CELL_CAP
  int64_t nqb;            // workgroups of the count / fill kernels
};

inline int64_t ball_cells_on_axis(double extent, double h) {
  if (!(extent > 0.0)) return 1;
  const double q = std::floor(extent / h);
  if (!(q < (double)(BALL_AXIS_CAP - 1))) return BALL_AXIS_CAP;
  return (int64_t)q + 1;
}

// lo / hi: the bounding box, d entries each (finite, lo <= hi); epsilon >= 0 (+inf included)
inline BallPlan ball_make_plan(int64_t n, int d, double epsilon, const double* lo, const double* hi) {
  BallPlan p{};
  const double hmin = std::max(epsilon * BALL_H_MARGIN, BALL_H_MIN);
  p.g = std::min(d, BALL_GRID_AXES);
  // the g coordinates with the most cells (ties: the lower coordinate), ...
  int best[3] = {-1, -1, -1};
  for (int a = 0; a < p.g; ++a) {
    for (int f = 0; f < d; ++f) {
      if (f == best[0] || f == best[1]) continue;
      if (best[a] < 0 || hi[f] - lo[f] > hi[best[a]] - lo[best[a]]) best[a] = f;
    }
  }
  // ... the one with the most cells last: a block of consecutive sorted rows then spans few cells on the other axes
  for (int a = 0; a < p.g; ++a) {
    const int f = best[p.g - 1 - a];
    p.axis[a] = f;
    p.lo[a] = lo[f];
    const double extent = hi[f] - lo[f];
    // an axis longer than BALL_AXIS_CAP cells of side hmin gets wider cells
    p.h[a] = std::max(hmin, extent / (double)(BALL_AXIS_CAP - 2));
    p.nc[a] = ball_cells_on_axis(extent, p.h[a]);
  }
  for (int a = p.g; a < 3; ++a) {
    p.axis[a] = 0;
    p.lo[a] = 0.0;
    p.h[a] = 1.0;
    p.nc[a] = 1;
  }
  p.coarsened = 0;
  // more cells than a few per point prune nothing more and cost a histogram and a scan of their own
  const double cap = (double)std::min<int64_t>(BALL_CELL_CAP, std::max<int64_t>(1024, 4 * n));
  for (;;) {
    double prod = 1.0;
    int active = 0;
    for (int a = 0; a < p.g; ++a) {
      prod *= (double)p.nc[a];
      active += p.nc[a] > 1;
    }
    if (prod <= cap || active == 0) break;
    const double f = std::pow(prod / cap, 1.0 / active) * 1.02;
    for (int a = 0; a < p.g; ++a) {
      if (p.nc[a] <= 1) continue;
      p.h[a] *= f;
      p.nc[a] = ball_cells_on_axis(hi[p.axis[a]] - lo[p.axis[a]], p.h[a]);
    }
    ++p.coarsened;
  }
  // the last axis in use runs fastest; the axes beyond g have one cell and no stride
  p.ncells = 1;
  for (int a = p.g - 1; a >= 0; --a) {
    p.stride[a] = p.ncells;
    p.ncells *= p.nc[a];
  }
  for (int a = p.g; a < 3; ++a) p.stride[a] = 0;
  p.nqb = (n + BALL_BQ - 1) / BALL_BQ;
  return p;
}

// the cell coordinate of x on grid axis a (the expression the kernels use, restated for the host check)
inline int64_t ball_cell_coord(const BallPlan& p, int a, double x) {
  const double t = std::floor((x - p.lo[a]) / p.h[a]);
  if (!(t > 0.0)) return 0;
  if (t >= (double)(p.nc[a] - 1)) return p.nc[a] - 1;
  return (int64_t)t;
}
