// Stand-alone host program for csrc/cc_plan.h (tests/test_components_host.py builds and runs it; it may be built with
// -fsanitize=address,undefined): the sequential restatement of glx_components -- init, union by minimum with path halving, flatten,
// number -- on graphs generated here, against a plain breadth-first search that numbers the components by their smallest vertex.
// Also: the row-class split, the row-pointer check and the refusal of a column index out of range.  Prints one line per group and
// returns 0 when everything agrees.
#include "cc_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <utility>
#include <vector>

namespace {
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int32_t below(int64_t m) { return (int32_t)(next() % (uint64_t)m); }
};

struct Csr {
  int64_t n = 0;
  std::vector<int32_t> ptr, col;
};

// rows in the order the pairs arrive (unsorted, duplicates kept)
Csr from_pairs(int64_t n, const std::vector<std::pair<int32_t, int32_t>>& pairs) {
  Csr g;
  g.n = n;
  g.ptr.assign((size_t)n + 1, 0);
  for (auto& p : pairs) ++g.ptr[p.first + 1];
  for (int64_t i = 0; i < n; ++i) g.ptr[i + 1] += g.ptr[i];
  g.col.resize(pairs.size());
  std::vector<int32_t> at(g.ptr.begin(), g.ptr.end() - 1);
  for (auto& p : pairs) g.col[at[p.first]++] = p.second;
  return g;
}

// components of the undirected pattern by breadth-first search from 0, 1, 2, ...: numbered by their smallest vertex
int64_t bfs_components(const Csr& g, std::vector<int32_t>* labels) {
  std::vector<std::pair<int32_t, int32_t>> both;
  for (int64_t i = 0; i < g.n; ++i)
    for (int32_t e = g.ptr[i]; e < g.ptr[i + 1]; ++e) {
      both.push_back({(int32_t)i, g.col[e]});
      both.push_back({g.col[e], (int32_t)i});
    }
  const Csr s = from_pairs(g.n, both);
  labels->assign((size_t)g.n, -1);
  int32_t ncomp = 0;
  std::queue<int32_t> q;
  for (int64_t r = 0; r < g.n; ++r) {
    if ((*labels)[r] >= 0) continue;
    (*labels)[r] = ncomp;
    q.push((int32_t)r);
    while (!q.empty()) {
      const int32_t x = q.front();
      q.pop();
      for (int32_t e = s.ptr[x]; e < s.ptr[x + 1]; ++e)
        if ((*labels)[s.col[e]] < 0) {
          (*labels)[s.col[e]] = ncomp;
          q.push(s.col[e]);
        }
    }
    ++ncomp;
  }
  return ncomp;
}

int failures = 0;

void compare(const char* what, const Csr& g) {
  std::vector<int32_t> want, got((size_t)g.n);
  const int64_t nwant = bfs_components(g, &want);
  for (int wave_row : {CC_WAVE_ROW, 1, 3, 1 << 30}) {      // the library's split, every row long, a low threshold, every row short
    std::fill(got.begin(), got.end(), -7);
    const int64_t ngot = cc_host_components(g.n, g.ptr.data(), g.col.data(), got.data(), wave_row);
    if (ngot != nwant || got != want) {
      std::printf("FAIL %s (n=%lld, threshold %d): %lld components, expected %lld\n", what, (long long)g.n, wave_row, (long long)ngot,
                  (long long)nwant);
      ++failures;
    }
  }
}

Csr random_graph(Rng& rng, int64_t n, double mean_degree, int variant) {
  std::vector<std::pair<int32_t, int32_t>> pairs;
  const int64_t m = (int64_t)(mean_degree * (double)n / 2 + 0.5);
  for (int64_t q = 0; q < m; ++q) {
    int32_t a = rng.below(n), b = rng.below(n);
    if (variant == 3 && q % 7 == 0) b = a;                      // self loops
    if (variant == 1 && a > b) std::swap(a, b);                 // upper triangle only
    pairs.push_back({a, b});
    if (variant == 0 || variant == 3) pairs.push_back({b, a});  // symmetric
    if (variant == 2 && q % 3 == 0) pairs.push_back({a, b});    // asymmetric, with duplicates
  }
  return from_pairs(n, pairs);
}
}  // namespace

int main() {
  Rng rng{20240611};
  int graphs = 0;
  for (int64_t n : {1, 2, 3, 63, 64, 65, 257, 1000, 4097})
    for (double deg : {0.0, 0.5, 1.0, 2.0, 4.0})
      for (int variant = 0; variant < 4; ++variant) {
        compare("random", random_graph(rng, n, deg, variant));
        ++graphs;
      }
  std::printf("random: %d graphs\n", graphs);

  {  // long diameters: the path in index order, the same path under a permutation, a ring, a grid
    const int32_t n = 65536;
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int32_t i = 0; i + 1 < n; ++i) {
      pairs.push_back({i, i + 1});
      pairs.push_back({i + 1, i});
    }
    compare("path", from_pairs(n, pairs));
    std::vector<int32_t> perm((size_t)n);
    for (int32_t i = 0; i < n; ++i) perm[i] = i;
    for (int32_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[rng.below(i + 1)]);
    for (auto& p : pairs) p = {perm[p.first], perm[p.second]};
    compare("permuted path", from_pairs(n, pairs));
    pairs.clear();
    for (int32_t i = 0; i < n; ++i) pairs.push_back({i, (i + 1) % n});
    compare("ring, one direction stored", from_pairs(n, pairs));
    pairs.clear();
    for (int32_t r = 0; r < 256; ++r)
      for (int32_t c = 0; c < 256; ++c) {
        if (c + 1 < 256) pairs.push_back({r * 256 + c, r * 256 + c + 1});
        if (r + 1 < 256) pairs.push_back({(r + 1) * 256 + c, r * 256 + c});
      }
    compare("grid", from_pairs(n, pairs));
    std::printf("long diameter: 4 graphs\n");
  }

  {  // hubs: stars at both ends, a clique beside isolated vertices, rows around the threshold
    for (int hub_last = 0; hub_last < 2; ++hub_last) {
      const int32_t n = 5000, hub = hub_last ? n - 1 : 0;
      std::vector<std::pair<int32_t, int32_t>> pairs;
      for (int32_t i = 0; i < n; ++i)
        if (i != hub) {
          pairs.push_back({hub, i});
          pairs.push_back({i, hub});
        }
      compare("star", from_pairs(n, pairs));
    }
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int32_t i = 0; i < 300; ++i)
      for (int32_t j = 0; j < 300; ++j)
        if (i != j) pairs.push_back({i + 25, j + 25});          // 25 isolated vertices in front, 25 behind
    compare("clique and isolated vertices", from_pairs(350, pairs));
    for (int len : {CC_WAVE_ROW - 1, CC_WAVE_ROW, CC_WAVE_ROW + 1}) {
      // three rows of `len` entries whose neighbours are disjoint, stored in one direction only, and vertices nobody names
      const int32_t n = 3 * (len + 1) + 5;
      pairs.clear();
      for (int32_t r = 0; r < 3; ++r)
        for (int32_t q = 0; q < len; ++q) pairs.push_back({n - 1 - r, r * len + q});
      const Csr g = from_pairs(n, pairs);
      std::vector<int32_t> lng;
      cc_long_rows(g.n, g.ptr.data(), CC_WAVE_ROW, &lng);
      if (lng.size() != (len >= CC_WAVE_ROW ? 3u : 0u)) {
        std::printf("FAIL row classes: %zu long rows at length %d\n", lng.size(), len);
        ++failures;
      }
      compare("rows around the threshold", g);
    }
    std::printf("hubs: 6 graphs\n");
  }

  {  // the checks
    const int32_t ptr_ok[4] = {0, 2, 2, 3}, ptr_dec[4] = {0, 2, 1, 3}, ptr_first[4] = {1, 2, 2, 3};
    int32_t col[3] = {1, 2, 0}, labels[3];
    if (cc_check_rowptr(3, 3, ptr_ok) != 0 || cc_check_rowptr(3, 3, ptr_dec) != 2 || cc_check_rowptr(3, 3, ptr_first) != 5 ||
        cc_check_rowptr(3, 4, ptr_ok) != 5) {
      std::printf("FAIL row-pointer check\n");
      ++failures;
    }
    if (cc_host_components(3, ptr_ok, col, labels) != 1) {
      std::printf("FAIL three vertices in one component\n");
      ++failures;
    }
    for (int32_t bad : {3, -1}) {
      col[1] = bad;
      if (cc_host_components(3, ptr_ok, col, labels) != -1) {
        std::printf("FAIL column index %d accepted\n", bad);
        ++failures;
      }
    }
    std::printf("checks: done\n");
  }
  if (failures) {
    std::printf("cc_plan_host: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("cc_plan_host: ok\n");
  return 0;
}
