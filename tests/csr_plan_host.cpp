// csrc/csr_plan.h on the host, behind a C interface for tests/test_csr_plan_host.py: g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.
// With -DCSR_PLAN_MAIN it is a stand-alone program that walks a small matrix through every function (for a host sanitizer run:
// g++ -fsanitize=address,undefined -DCSR_PLAN_MAIN).
#include "csr_plan.h"
#include <cstring>

extern "C" {

// the codes the test's walk answers: the walk's own three, then one per hook
enum { WALK_PTR = 12, WALK_COL = 13, WALK_CANON = 14, HOOK_BEFORE = 21, HOOK_ENTRY = 22, HOOK_AFTER = 23 };

// The walk with hooks that refuse row `before_at`, entry `entry_at` and row `after_at` (-1: nothing) and count how often they are
// asked: counts[0 .. 3) = before, entry, after; counts[3] = the entries the before hooks were promised.
int csr_host_walk(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, int64_t before_at, int64_t entry_at, int64_t after_at,
                  int64_t* counts, char* msg, int cap) {
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  msg[0] = 0;
  return csr_walk(
      n, M, row_ptr, col, WALK_PTR, WALK_COL, WALK_CANON, msg, (size_t)cap,
      [&](int64_t i, int64_t count) {
        ++counts[0];
        counts[3] += count;
        if (i != before_at) return 0;
        snprintf(msg, (size_t)cap, "before row %lld with %lld entries", (long long)i, (long long)count);
        return (int)HOOK_BEFORE;
      },
      [&](int64_t i, int64_t e) {
        ++counts[1];
        if (e != entry_at) return 0;
        snprintf(msg, (size_t)cap, "entry %lld of row %lld", (long long)e, (long long)i);
        return (int)HOOK_ENTRY;
      },
      [&](int64_t i) {
        ++counts[2];
        if (i != after_at) return 0;
        snprintf(msg, (size_t)cap, "after row %lld", (long long)i);
        return (int)HOOK_AFTER;
      });
}

// the walk of a solver with a rule per entry only
int csr_host_walk_entries(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, int64_t entry_at, char* msg, int cap) {
  msg[0] = 0;
  return csr_walk(n, M, row_ptr, col, WALK_PTR, WALK_COL, WALK_CANON, msg, (size_t)cap, [&](int64_t, int64_t e) {
    if (e != entry_at) return 0;
    snprintf(msg, (size_t)cap, "entry %lld", (long long)e);
    return (int)HOOK_ENTRY;
  });
}

int csr_host_check_vertices(const int32_t* ind, int64_t m, int64_t n, int code, const char* noun, char* msg, int cap) {
  msg[0] = 0;
  return csr_check_vertices(ind, m, n, code, noun, msg, (size_t)cap);
}

void csr_host_label_rows(int64_t n, int64_t m, const int32_t* ind, int32_t* lab) {
  const std::vector<int32_t> l = csr_label_rows(n, m, ind);
  if (n > 0) memcpy(lab, l.data(), (size_t)n * sizeof(int32_t));
}

// out: (first column, columns) per tile by col_tile, then the same by col_tile_at; info: ntiles, ct; returns ntiles (at most cap tiles
// are written)
int csr_host_tiles(int k, int width, int32_t* out, int32_t* out_at, int cap, int32_t* ct_out) {
  int nt, ct;
  col_tiles(k, width, &nt, &ct);
  *ct_out = ct;
  for (int t = 0; t < nt && t < cap; ++t) {
    int c0, cols;
    col_tile(k, width, t, &c0, &cols);
    out[2 * t] = c0;
    out[2 * t + 1] = cols;
    const ColTile a = col_tile_at(t, k / nt, k % nt);
    out_at[2 * t] = a.c0;
    out_at[2 * t + 1] = a.cols;
  }
  return nt;
}
}

#ifdef CSR_PLAN_MAIN
int main() {
  // rows 0: (1, 2), 1: (0), 2: (), 3: (0, 3)
  const int64_t row_ptr[5] = {0, 2, 3, 3, 5};
  const int32_t col[5] = {1, 2, 0, 0, 3};
  int64_t counts[4];
  char msg[128];
  if (csr_host_walk(4, 5, row_ptr, col, -1, -1, -1, counts, msg, sizeof msg) || counts[0] != 4 || counts[1] != 5 || counts[2] != 4) return 1;
  if (csr_host_walk(4, 5, row_ptr, col, -1, 4, -1, counts, msg, sizeof msg) != HOOK_ENTRY) return 2;
  if (csr_host_walk_entries(4, 5, row_ptr, col, -1, msg, sizeof msg)) return 3;
  const int32_t ind[3] = {3, 0, 3};
  int32_t lab[4];
  if (csr_host_check_vertices(ind, 3, 4, 7, "training", msg, sizeof msg) || csr_host_check_vertices(ind, 3, 3, 7, "training", msg, sizeof msg) != 7)
    return 4;
  csr_host_label_rows(4, 3, ind, lab);
  if (lab[0] != 1 || lab[1] != -1 || lab[2] != -1 || lab[3] != 2) return 5;
  int32_t tiles[2 * 16], tiles_at[2 * 16], ct;
  if (csr_host_tiles(33, 16, tiles, tiles_at, 16, &ct) != 3 || ct != 11 || memcmp(tiles, tiles_at, 6 * sizeof(int32_t)) || tiles[4] != 22) return 6;
  printf("ok %s\n", msg);
  return 0;
}
#endif
