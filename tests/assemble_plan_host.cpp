// csrc/assemble_plan.h on the host, behind a C interface for tests/test_assemble_host.py:
// g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared.
#include <algorithm>
#include <utility>
#include <vector>
#include "assemble_plan.h"

extern "C" {

// out[0 .. 3): entries of a register row, of a wavefront row, of the smallest hub scratch
void asm_host_constants(int* out) {
  out[0] = REG_CAP;
  out[1] = ROW_CAP;
  out[2] = HUB_FLOOR;
}

int asm_host_row_class(int k, int64_t M) { return asm_row_class(k, M); }
int64_t asm_host_hub_scratch(int64_t M) { return asm_hub_scratch(M); }
int64_t asm_host_row_slot(int64_t i, int k, int sym, int64_t roff_i) { return asm_row_slot(i, k, sym, roff_i); }

unsigned long long asm_host_key(unsigned col, unsigned kind, unsigned pos, unsigned lane) { return asm_key(col, kind, pos, lane); }

// out[0 .. 4): column, kind, position, lane
void asm_host_unpack(unsigned long long key, unsigned* out) {
  out[0] = (unsigned)asm_key_col(key);
  out[1] = asm_key_kind(key);
  out[2] = asm_key_pos(key);
  out[3] = asm_key_lane(key);
}

// The assembly of n rows from lists (ind, w: n x k) as the kernels do it, one row after the other: the row's list entries and the
// entries of all lists that name it (in list order: row after row, neighbour after neighbour), keyed by asm_key with `lanes`
// (any six bits per entry) in the free bits, sorted by std::sort, asm_segment at every position.  indices / data: room for 2 n k.
// Returns the number of entries.
int64_t asm_host_assemble(const int64_t* ind, const double* w, int64_t n, int k, int sym, const unsigned char* lanes, int32_t* indptr,
                          int32_t* indices, double* data) {
  std::vector<std::vector<std::pair<unsigned long long, double>>> rows(n);
  for (int64_t i = 0; i < n; ++i)
    for (int t = 0; t < k; ++t) {
      const int64_t e = i * k + t, j = ind[e];
      rows[i].push_back({asm_key((unsigned)j, ASM_KIND_FORWARD, (unsigned)t, lanes[e] & 63u), w[e]});
      if (sym != SYM_NONE) rows[j].push_back({asm_key((unsigned)i, ASM_KIND_REVERSE, (unsigned)t, lanes[n * k + e] & 63u), w[e]});
    }
  int64_t nnz = 0;
  indptr[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    auto& row = rows[i];
    std::sort(row.begin(), row.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    const int64_t M = (int64_t)row.size();
    std::vector<unsigned long long> key(M);
    std::vector<double> val(M);
    for (int64_t e = 0; e < M; ++e) {
      key[e] = row[e].first;
      val[e] = row[e].second;
    }
    for (int64_t e = 0; e < M; ++e) {
      int c = 0;
      double v = 0.0;
      if (asm_segment(key.data(), val.data(), e, M, (int)i, sym, &c, &v)) {
        indices[nnz] = c;
        data[nnz++] = v;
      }
    }
    indptr[i + 1] = (int32_t)nnz;
  }
  return nnz;
}
}
