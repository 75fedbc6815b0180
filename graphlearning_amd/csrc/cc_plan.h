// What the host decides for graph.connected_components (glx_components, cc.hip), and the algorithm itself in a form that compiles
// for the host: union by minimum with path halving, flatten, number.  No HIP header: tests/cc_plan_host.cpp is a stand-alone program
// that runs this file on graphs it generates and compares with a breadth-first search.
//
// One text, two memories.  cc_find and cc_union are templates over the way parent[] is touched: the kernels of cc.hip instantiate them
// with relaxed agent-scope atomics (CcAtomicParent there), the host with plain loads and stores (CcPlainParent here).  The host run is
// one interleaving of the device's -- every entry processed to its end before the next begins --, and the result does not depend on
// the interleaving (the argument heads cc.hip), so cc_host_components IS the result of glx_components, label for label.
//
// Row classes.  A row shorter than the threshold is processed by one thread, entry after entry; a row at or above it by one wavefront
// whose 64 lanes stride the entries.  The thread-per-row kernel runs over all n rows and skips the long ones; the long ones are listed
// (cc_long_rows) and the list is the wavefront kernel's grid.
//
// CC_WAVE_ROW = 1024, from what profiles/components.txt measured on the MI355X (thresholds 8 .. 4096 and "never" on every graph):
//   - a thread walks its row at 0.64 us per entry (every step is a chain of dependent agent-scope loads): the 70 000-vertex kNN graph
//     plus ONE vertex joined to all others takes 44.8 ms with that row on a thread and 1.8 ms with it on a wavefront.  A row of 1024
//     entries holds its thread for 0.66 ms -- as long as all kernels take on the 70 000-vertex graph; no longer row may stay there.
//   - below that the thread class won wherever the wavefront class was tried on rows of a graph: epsilon-ball graphs with rows of
//     38 .. 198 and of 148 .. 688 entries run 12 x and 7 x SLOWER with their rows on wavefronts (64 lanes of one row hook into the
//     same few roots at once and retry), the 70 000-vertex kNN graphs (rows of 10 .. 138) are indifferent to any threshold from 32 up.
//   - the 10^6-vertex kNN graph is the one case measured where wavefronts for ALL rows (threshold 8) beat threads, 1.2 ms against
//     4.6 ms; no threshold on the row length expresses that, and a narrower lane group for short rows is not built.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define CC_FN __host__ __device__ __forceinline__
#else
#define CC_FN inline
#endif

static const int CC_WAVE_ROW = 1024;        // rows of at least this many stored entries take a wavefront
static const int CC_SCAN_TILE = 1024;       // vertices per workgroup of the numbering's prefix sum (256 threads x 4)

// parent[] of the host: plain memory
struct CcPlainParent {
  int32_t* p;
  int32_t load(int32_t i) const { return p[i]; }
  void store(int32_t i, int32_t v) const { p[i] = v; }
  // parent[i] <- desired if it holds expected; returns what it held
  int32_t cas(int32_t i, int32_t expected, int32_t desired) const {
    const int32_t old = p[i];
    if (old == expected) p[i] = desired;
    return old;
  }
};

// The root above x, with path halving: every vertex looked at is re-pointed to its grandparent.  The walk visits strictly
// decreasing indices (parent[y] < y for every non-root y), so it ends after at most x steps whatever else happens.
template <class P>
CC_FN int32_t cc_find(const P& parent, int32_t x) {
  int32_t p = parent.load(x);
  while (p != x) {
    const int32_t gp = parent.load(p);
    if (gp == p) return p;
    parent.store(x, gp);          // gp is an ancestor of x and stays one; x is no root and never becomes one again
    x = gp;
    p = parent.load(x);
  }
  return x;
}

// u and v end in one tree: the larger of the two roots is hooked under the smaller.  A compare-and-swap that fails returns what the
// root was re-pointed to meanwhile -- strictly below it --, and the search goes on from there: max(ru, rv) falls with every failure.
template <class P>
CC_FN void cc_union(const P& parent, int32_t u, int32_t v) {
  int32_t ru = cc_find(parent, u), rv = cc_find(parent, v);
  while (ru != rv) {
    const int32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    const int32_t old = parent.cas(hi, hi, lo);
    if (old == hi) return;
    ru = cc_find(parent, old);
    rv = lo;
  }
}

// init: a vertex starts under the first smaller neighbour among the first CC_INIT_LOOK entries of its row, or as its own root
static const int CC_INIT_LOOK = 8;
CC_FN int32_t cc_first_parent(int32_t i, const int32_t* col, int32_t e0, int32_t e1) {
  const int32_t end = e1 - e0 > CC_INIT_LOOK ? e0 + CC_INIT_LOOK : e1;
  for (int32_t e = e0; e < end; ++e)
    if (col[e] < i) return col[e];
  return i;
}

// the row-pointer conditions every kernel relies on: 0 = fine, else 1 + the first offending row (n + 1: the ends do not span nnz)
inline int64_t cc_check_rowptr(int64_t n, int64_t nnz, const int32_t* rowptr) {
  if (rowptr[0] != 0 || rowptr[n] != nnz) return n + 2;
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i] > rowptr[i + 1]) return i + 1;
  return 0;
}

// the rows of the wavefront class, ascending (rowptr has passed cc_check_rowptr)
inline void cc_long_rows(int64_t n, const int32_t* rowptr, int wave_row, std::vector<int32_t>* rows) {
  rows->clear();
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] - rowptr[i] >= wave_row) rows->push_back((int32_t)i);
}

// The whole computation on the host, in the device's stages: init, union (short rows, then the listed long ones -- any order gives
// the same labels), flatten, number.  labels (n) <- scipy's numbering: components in the order of their smallest vertex.  Returns
// the number of components, or -1 for a column index outside [0, n) (the device's check pass).
inline int64_t cc_host_components(int64_t n, const int32_t* rowptr, const int32_t* col, int32_t* labels, int wave_row = CC_WAVE_ROW) {
  const int64_t nnz = rowptr[n];
  for (int64_t e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= n) return -1;
  std::vector<int32_t> par((size_t)n), root((size_t)n), rank((size_t)n), lng;
  cc_long_rows(n, rowptr, wave_row, &lng);
  const CcPlainParent parent{par.data()};
  for (int64_t i = 0; i < n; ++i) par[i] = cc_first_parent((int32_t)i, col, rowptr[i], rowptr[i + 1]);
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] - rowptr[i] >= wave_row) continue;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
      if (col[e] != i) cc_union(parent, (int32_t)i, col[e]);
  }
  for (int32_t i : lng)
    for (int lane = 0; lane < 64; ++lane)                    // the lanes stride the entries (64-bit e: e + 64 may pass 2^31)
      for (int64_t e = (int64_t)rowptr[i] + lane; e < rowptr[i + 1]; e += 64)
        if (col[e] != i) cc_union(parent, i, col[e]);
  for (int64_t i = 0; i < n; ++i) root[i] = cc_find(parent, (int32_t)i);      // flatten
  int32_t run = 0;                                            // number: exclusive prefix sum of the root flags
  for (int64_t i = 0; i < n; ++i) {
    rank[i] = run;
    run += root[i] == i;
  }
  for (int64_t i = 0; i < n; ++i) labels[i] = rank[root[i]];
  return run;
}
