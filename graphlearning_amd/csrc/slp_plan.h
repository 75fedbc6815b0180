// What the host derives for the sparse-label-propagation sweeps (slp.hip) before the device runs one: the checks of the caller's
// arrays, the reverse-entry index and the column tiling.  No HIP header: tests/test_slp_host.py builds it on the host
// (tests/slp_plan_host.cpp), where slp_host_reference also walks the contract itself entry by entry.
//
// The reverse-entry index.  The divergence of the edge field Y at vertex i needs, beside Y[e] of every entry e = (i, j) of row i, the
// value on the entry (j, i) of the transposed pattern: rev[e] is that entry's index, -1 where W has none (a directed graph), and e
// itself on the diagonal.  W is canonical -- columns ascending inside a row -- so W and its transpose merge in one pass without a hash:
// walking the rows i in ascending order, the entries (j, i) that are looked up in a given row j arrive with ascending i, hence one
// cursor per row that only moves forward finds them all: O(M) steps in total.
//
// The column tiling.  The state is stored class columns contiguous: Y (M, cpad), u and ut (n, cpad), so that a gathered record
// Y[rev[e]] or ut[j] is one 128-byte line for up to 16 columns (cpad: the tile's columns rounded up to 1, 2, 4, 8 or 16 doubles, a
// record never straddles a line).  More than SLP_TILE columns run tile after tile, each tile a complete solve of its columns -- the
// columns are independent, so the result does not depend on the tiling --, by the tile rule of csr_plan.h.
#pragma once
#include "csr_plan.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

static const int SLP_TILE = 16;            // columns per tile at most: 16 doubles = one 128-byte line per gathered record
static const int SLP_BLOCK = 256;          // threads per workgroup of both kernels
static const int SLP_CHUNK = 16;           // iterations per captured launch sequence

struct SlpTile {
  int32_t c0, cols, cpad;                  // columns [c0, c0 + cols) of the caller's C; record width in doubles
};

inline std::vector<SlpTile> slp_tiles(int C) {
  std::vector<SlpTile> t;
  if (C < 1) return t;
  int nt, ct;
  col_tiles(C, SLP_TILE, &nt, &ct);
  for (int q = 0; q < nt; ++q) {
    int c0, cols, cpad = 1;
    col_tile(C, SLP_TILE, q, &c0, &cols);
    while (cpad < cols) cpad *= 2;
    t.push_back({(int32_t)c0, (int32_t)cols, (int32_t)cpad});
  }
  return t;
}

// 0 if the arrays are what the contract accepts, else a message in `msg` (room for `cap` characters) and a nonzero value:
// 1 sizes or C, 2 row pointers, 3 an empty row, 4 a column index out of range, 5 columns of a row not strictly ascending,
// 6 a weight not finite or not > 0, 7 lam or gamma not finite, 8 a labelled vertex out of range
inline int slp_validate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                        const double* gamma, int C, int64_t m, const int32_t* ind, char* msg, size_t cap) {
  if (n < 1 || n > 0x7fffffffll || M < 0 || M > 0x7fffffffll || m < 0 || C < 1) {
    snprintf(msg, cap, "bad sizes (n=%lld M=%lld m=%lld C=%d; n and M at most 2^31 - 1)", (long long)n, (long long)M, (long long)m, C);
    return 1;
  }
  const int bad = csr_walk(
      n, M, row_ptr, col, 2, 4, 5, msg, cap,
      [&](int64_t i, int64_t count) {
        if (count > 0) return 0;
        snprintf(msg, cap, "vertex %lld has no stored entry (its degree is zero: the update divides by it)", (long long)i);
        return 3;
      },
      [&](int64_t, int64_t e) {
        if (!(std::isfinite(W[e]) && W[e] > 0)) {
          snprintf(msg, cap, "weight %g of entry %lld is not finite and > 0", W[e], (long long)e);
          return 6;
        }
        if (!std::isfinite(lam[e])) {
          snprintf(msg, cap, "lam %g of entry %lld is not finite", lam[e], (long long)e);
          return 7;
        }
        return 0;
      },
      [&](int64_t i) {
        if (std::isfinite(gamma[i])) return 0;
        snprintf(msg, cap, "gamma %g of vertex %lld is not finite", gamma[i], (long long)i);
        return 7;
      });
  return bad ? bad : csr_check_vertices(ind, m, n, 8, "labelled", msg, cap);
}

// rev[e] for every entry of a canonical W (validated: slp_validate); M <= 2^31 - 1
inline void slp_reverse_index(int64_t n, const int64_t* row_ptr, const int32_t* col, int32_t* rev) {
  std::vector<int64_t> cursor(row_ptr, row_ptr + n);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int32_t j = col[e];
      int64_t& c = cursor[j];
      const int64_t end = row_ptr[(int64_t)j + 1];
      while (c < end && col[c] < i) ++c;
      rev[e] = (c < end && col[c] == i) ? (int32_t)c : -1;
    }
}

inline std::vector<int32_t> slp_label_rows(int64_t n, int64_t m, const int32_t* ind) { return csr_label_rows(n, m, ind); }

// The contract on the host, one column after another, entry by entry (compiled with -ffp-contract=off): what the device must equal.
inline void slp_host_reference(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                               const double* gamma, const int32_t* rev, int C, const int32_t* lab, const double* val, int64_t T,
                               double* u_out) {
  std::vector<double> u((size_t)n), ut((size_t)n), Y((size_t)M);
  for (int c = 0; c < C; ++c) {
    u.assign((size_t)n, 0.0);
    Y.assign((size_t)M, 0.0);
    for (int64_t t = 0; t < T; ++t) {
      for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
          const double back = rev[e] >= 0 ? Y[rev[e]] : 0.0;
          const double d = Y[e] - back;
          const double p = d * W[e];
          s = s + p;
        }
        const double h = s / 2.0;
        const double div = 2.0 * h;
        const double g = gamma[i] * div;
        const double z = 0.0 + g;
        double un = u[i] - z;
        if (lab[i] >= 0) un = val[(int64_t)lab[i] * C + c];
        const double tw = 2.0 * un;
        ut[i] = tw - u[i];
        u[i] = un;
      }
      for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
          const double d = ut[col[e]] - ut[i];
          const double p = W[e] * d;
          const double q = -p;
          const double r = q * lam[e];
          const double y = Y[e] + r;
          Y[e] = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);
        }
    }
    for (int64_t i = 0; i < n; ++i) u_out[i * C + c] = u[i];
  }
}
