// The level plan of an in-order Gauss-Seidel sweep (lip.hip): what the host derives from the row-sorted entry list of a graph and a
// boundary mask before the device runs a sweep.  No HIP header: tests/test_amle_host.py builds it on the host (tests/lip_plan_host.cpp).
//
// Why levels keep the iterates.  The reference's sweep (c_code/lp_iterate.cpp:159-176, :220-248) visits the vertices i = 0 .. n-1 and
// overwrites u[i] in place with a function of the values u[j] of row i's stored entries.  Vertex i therefore reads the NEW value of
// every non-boundary j < i among its entries and the OLD value of every j > i.  A schedule gives the same bits iff, for every pair of
// different non-boundary vertices i < k with an entry (i, k) or (k, i),  i is written before k runs:
//   * entry (k, i), i < k: k reads i's new value -- i must have run;
//   * entry (i, k), i < k: i reads k's old value -- k must not have run yet.  This is the transposed pattern: on a directed graph
//     i may read k while k does not read i, and k must still wait.
// level[i] = 0 if no lower-numbered non-boundary vertex is adjacent to i in the pattern of W or of its transpose, else 1 + the largest
// level among those: the longest chain of such pairs that ends in i, the smallest assignment under which every pair is ordered.  Two
// vertices of one level are never adjacent, so they may run concurrently on the in-place array, each reading exactly what the
// sequential loop would read; levels run in ascending order.  Boundary vertices are never written and impose nothing; a diagonal
// entry reads the vertex's own old value and imposes nothing.
//
// One pass in index order over the entries does both patterns: vertex i first PULLS from its entries j < i (their levels are final),
// then, its level final, PUSHES level[i] + 1 to its entries k > i -- which is the pull of k along the transposed entry (i, k).
//
// The launch list.  A level of at most LIP_SMALL vertices is small.  A run of TWO OR MORE consecutive small levels becomes ONE launch
// of a single workgroup that walks its levels with a workgroup barrier between them (a path graph in index order, points sorted along
// an axis: hundreds of levels of a few vertices each); every other level -- a small one between two large ones included: merging a
// run of one saves no launch and would put its items on one compute unit -- is a launch of its own over a grid.  No grid-wide wait.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

static const int LIP_SMALL = 32;           // vertices; a level this small rides in a merged single-workgroup launch (EXPERIMENTS.md, "AMLE by levels")
static const int LIP_BLOCK = 256;          // threads per workgroup of the sweep kernels
static const int LIP_CHUNK = 16;           // sweeps enqueued between two reads of the error slots

struct LipLaunch {
  int32_t lvl0, lvl1;     // the levels [lvl0, lvl1) of this launch
  int32_t merged;         // 1: one workgroup walks the levels (two or more, all small); 0: lvl1 == lvl0 + 1, a grid over the level
};

struct LipPlan {
  std::vector<int32_t> level;         // per vertex; -1 on the boundary
  std::vector<int32_t> order;         // the non-boundary vertices by (level, index)
  std::vector<int64_t> lvl_ptr;       // level l = order[lvl_ptr[l] .. lvl_ptr[l + 1])
  std::vector<LipLaunch> launches;    // one sweep, in order
  int64_t nlevels = 0;
};

// row_ptr (n + 1), nbr: the stored entries by vertex, indices in [0, n); bdy[i] != 0: boundary vertex.  small < 0: LIP_SMALL;
// small = 0: nothing is merged.
inline LipPlan lip_make_plan(int64_t n, const int64_t* row_ptr, const int32_t* nbr, const unsigned char* bdy, int small = -1) {
  if (small < 0) small = LIP_SMALL;
  LipPlan p;
  p.level.assign((size_t)n, 0);
  int32_t top = -1;
  for (int64_t i = 0; i < n; ++i) {
    if (bdy[i]) {
      p.level[i] = -1;
      continue;
    }
    int32_t li = p.level[i];            // what lower-numbered vertices pushed along the transposed pattern
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int32_t j = nbr[e];
      if (j < i && !bdy[j] && p.level[j] + 1 > li) li = p.level[j] + 1;
    }
    p.level[i] = li;
    if (li > top) top = li;
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int32_t k = nbr[e];
      if (k > i && !bdy[k] && p.level[k] < li + 1) p.level[k] = li + 1;
    }
  }
  p.nlevels = (int64_t)top + 1;
  p.lvl_ptr.assign((size_t)p.nlevels + 1, 0);
  for (int64_t i = 0; i < n; ++i)
    if (p.level[i] >= 0) ++p.lvl_ptr[(size_t)p.level[i] + 1];
  for (int64_t l = 0; l < p.nlevels; ++l) p.lvl_ptr[l + 1] += p.lvl_ptr[l];
  p.order.resize((size_t)p.lvl_ptr[p.nlevels]);
  {
    std::vector<int64_t> at(p.lvl_ptr.begin(), p.lvl_ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)       // ascending i inside a level
      if (p.level[i] >= 0) p.order[(size_t)at[p.level[i]]++] = (int32_t)i;
  }
  for (int64_t l = 0; l < p.nlevels;) {
    const bool is_small = p.lvl_ptr[l + 1] - p.lvl_ptr[l] <= small;
    int64_t l1 = l + 1;
    if (is_small)
      while (l1 < p.nlevels && p.lvl_ptr[l1 + 1] - p.lvl_ptr[l1] <= small) ++l1;
    p.launches.push_back({(int32_t)l, (int32_t)l1, l1 - l >= 2 ? 1 : 0});
    l = l1;
  }
  return p;
}
