// The front end that the one-call learners share (slp, ck, dlp, eig, mmbo): the walk over a canonical CSR matrix, the
// range check of a vertex list, the training-row map and the column-tile rule, each written once.  No HIP header: the plan headers
// include this file and are built on the host by the tests (tests/csr_plan_host.cpp tests this one by itself).
//
// Canonical CSR.  n rows, M stored entries, row pointers from 0 to M and ascending, every column index in [0, n), the columns of a row
// strictly ascending (sorted, no duplicate).  What a stored value may be is the solver's own rule: it hands the walk a hook.
//
// The column tiles.  k columns in tiles of at most `width`: ceil(k / width) tiles, their widths within one of each other, the widest
// first.  With tbase = k / ntiles and textra = k % ntiles, tile t starts at t * tbase + min(t, textra) and holds tbase + (t < textra)
// columns; a kernel gets (ct, tbase, textra), ct the widest tile's columns, and asks col_tile_at for its own tile.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define CSR_HOST_DEVICE __host__ __device__
#else
#define CSR_HOST_DEVICE
#endif

// One pass over the rows and their entries.  Answers 0, or writes `msg` (room for `cap` characters) and answers code_ptr (row
// pointers), code_col (a column index out of range) or code_canon (the columns of a row not strictly ascending), or what a hook
// answered.  The hooks return 0, or write `msg` and return their own code; in the order they are asked:
//   before(i, count)   once per row, ahead of its `count` entries
//   entry(i, e)        per entry, after the entry's column index passed both checks
//   after(i)           once per row, behind its entries
// The first fault in this order, rows ascending and entries ascending, is the one answered.
template <class Before, class Entry, class After>
inline int csr_walk(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, int code_ptr, int code_col, int code_canon, char* msg,
                    size_t cap, Before before, Entry entry, After after) {
  if (row_ptr[0] != 0 || row_ptr[n] != M) {
    snprintf(msg, cap, "row pointers run from %lld to %lld, expected 0 to M=%lld", (long long)row_ptr[0], (long long)row_ptr[n], (long long)M);
    return code_ptr;
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
    if (e1 < e0 || e1 > M) {
      snprintf(msg, cap, "row pointers of vertex %lld are not ascending within [0, M]", (long long)i);
      return code_ptr;
    }
    if (const int bad = before(i, e1 - e0)) return bad;
    for (int64_t e = e0; e < e1; ++e) {
      if (col[e] < 0 || col[e] >= n) {
        snprintf(msg, cap, "column index %d of entry %lld out of range", col[e], (long long)e);
        return code_col;
      }
      if (e > e0 && col[e - 1] >= col[e]) {
        snprintf(msg, cap, "row %lld is not canonical: its columns are not strictly ascending (entry %lld)", (long long)i, (long long)e);
        return code_canon;
      }
      if (const int bad = entry(i, e)) return bad;
    }
    if (const int bad = after(i)) return bad;
  }
  return 0;
}

// the walk of a solver that has a rule per entry only
template <class Entry>
inline int csr_walk(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, int code_ptr, int code_col, int code_canon, char* msg,
                    size_t cap, Entry entry) {
  return csr_walk(n, M, row_ptr, col, code_ptr, code_col, code_canon, msg, cap, [](int64_t, int64_t) { return 0; }, entry,
                  [](int64_t) { return 0; });
}

// 0 if vertex v is one of the n, else "<noun> vertex v out of range" in `msg` and `code`
inline int csr_check_vertex(int32_t v, int64_t n, int code, const char* noun, char* msg, size_t cap) {
  if (v >= 0 && v < n) return 0;
  snprintf(msg, cap, "%s vertex %d out of range", noun, v);
  return code;
}
// the same for a list of m vertices: the first one out of range is answered
inline int csr_check_vertices(const int32_t* ind, int64_t m, int64_t n, int code, const char* noun, char* msg, size_t cap) {
  for (int64_t q = 0; q < m; ++q)
    if (const int bad = csr_check_vertex(ind[q], n, code, noun, msg, cap)) return bad;
  return 0;
}

// lab[i] = the row of `val` vertex i takes, -1 where it is not listed; a vertex listed twice takes its last row
inline std::vector<int32_t> csr_label_rows(int64_t n, int64_t m, const int32_t* ind) {
  std::vector<int32_t> lab((size_t)n, -1);
  for (int64_t q = 0; q < m; ++q) lab[ind[q]] = (int32_t)q;
  return lab;
}

struct ColTile {
  int c0, cols;                            // the columns [c0, c0 + cols)
};

// tile `tile` of the tiling with tbase = k / ntiles, textra = k % ntiles: host and device
CSR_HOST_DEVICE inline ColTile col_tile_at(int tile, int tbase, int textra) {
  return {tile * tbase + (tile < textra ? tile : textra), tbase + (tile < textra ? 1 : 0)};
}

// the tiles of k >= 1 columns, at most `width` each: their number and the widest tile's columns
inline void col_tiles(int k, int width, int* ntiles, int* ct) {
  *ntiles = (k + width - 1) / width;
  *ct = (k + *ntiles - 1) / *ntiles;
}
// first column and width of tile t
inline void col_tile(int k, int width, int t, int* c0, int* cols) {
  int nt, ct;
  col_tiles(k, width, &nt, &ct);
  const ColTile a = col_tile_at(t, k / nt, k % nt);
  *c0 = a.c0;
  *cols = a.cols;
}
