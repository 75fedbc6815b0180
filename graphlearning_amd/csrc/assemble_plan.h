// The decisions of the weight-matrix assembly (assemble.hip), one definition each: which merge kernel a row belongs to, where its
// candidates sit in the scratch image, the sort key of an entry, and the rule that turns the sorted entries of one column into an
// entry of the matrix.  Bit-equality with the reference (graphlearning/weightmatrix.py:170-186) rests on the key's order --
// (column, kind, position in the source list): a column's forward entries are added in the order their row lists them, its reverse
// entries likewise -- and on asm_segment below.  No HIP header: tests/assemble_plan_host.cpp compiles it for the host and
// tests/test_assemble_host.py checks the row classes, the key order and the rule against scipy.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ASM_FN __host__ __device__ __forceinline__
#else
#define ASM_FN static inline
#endif

enum { SYM_NONE = 0, SYM_MEAN = 1, SYM_MAX = 2, SYM_SYMGAUSS = 3 };

// ---- rows ------------------------------------------------------------------------------------------------------------------------------
// M = the entries a row merges: its k list entries plus, when the matrix is symmetrised, every list entry that names it
static const int REG_CAP = 64;       // one entry per lane: merge_rows_small_kernel sorts in registers (lists of at most REG_CAP only)
static const int ROW_CAP = 1024;     // forward + reverse entries one wavefront merges in LDS: merge_rows_kernel
static const int HUB_FLOOR = 2048;   // the smallest global scratch of a hub row (one workgroup: merge_hub_kernel)
enum { ASM_ROW_REGISTER = 0, ASM_ROW_WAVEFRONT = 1, ASM_ROW_HUB = 2 };

ASM_FN int asm_row_class(int k, int64_t M) {
  if (k <= REG_CAP && M <= REG_CAP) return ASM_ROW_REGISTER;
  return M <= ROW_CAP ? ASM_ROW_WAVEFRONT : ASM_ROW_HUB;
}

// entries of a hub's sort scratch: the power of two the bitonic network needs
ASM_FN int64_t asm_hub_scratch(int64_t M) {
  int64_t P = HUB_FLOOR;
  while (P < M) P <<= 1;
  return P;
}

// Where row i's kept entries wait in the scratch image until the row pointers exist: room for all M candidates of every row, known
// without a scan.  roff_i = the reverse entries of the rows before i.
ASM_FN int64_t asm_row_slot(int64_t i, int k, int sym, int64_t roff_i) { return i * (int64_t)k + (sym == SYM_NONE ? 0 : roff_i); }

// ---- keys ------------------------------------------------------------------------------------------------------------------------------
// column (bits 32..63) | kind, 0 forward / 1 reverse (bit 22) | position in the source list (bits 6..21: k <= 65535) | six free bits,
// where the register kernel keeps the lane that holds the entry's value.  (column, kind, position) is unique within a row, so the
// free bits never decide a comparison; ~0 sorts behind every key (padding).
enum { ASM_KIND_FORWARD = 0, ASM_KIND_REVERSE = 1 };
ASM_FN unsigned long long asm_key(unsigned col, unsigned kind, unsigned pos, unsigned lane = 0) {
  return ((unsigned long long)col << 32) | ((unsigned long long)kind << 22) | ((unsigned long long)pos << 6) | lane;
}
ASM_FN int asm_key_col(unsigned long long key) { return (int)(key >> 32); }
ASM_FN unsigned asm_key_kind(unsigned long long key) { return (unsigned)(key >> 22) & 1u; }
ASM_FN unsigned asm_key_pos(unsigned long long key) { return (unsigned)(key >> 6) & 0xffffu; }
ASM_FN unsigned asm_key_lane(unsigned long long key) { return (unsigned)key & 63u; }

// ---- the rule --------------------------------------------------------------------------------------------------------------------------
// a = A[i,c] (forward, duplicates summed), b = A[c,i] (reverse)
ASM_FN double combine_entry(double a, double b, int sym) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (sym == SYM_NONE) return a;
  if (sym == SYM_MEAN) return (a + b) / 2.0;                                // (W + W^T)/2, weightmatrix.py:183
  if (sym == SYM_MAX) return (b > a) ? b : (((a + b) > 0.0) ? a : 0.0);     // utils.sparse_max(W, W^T), utils.py:263-286
  if (b > a) { const double s = a + b; return s - a; }                      // W + W^T*(W^T>W) - W*(W^T>W), weightmatrix.py:181
  return a;
}

// Entry e of a row's M sorted keys and values.  *col = its column; returns whether e yields an entry of the matrix, and then *v: e
// is the first of its column, the column's forward entries are added into a and its reverse entries into b in key order,
// combine_entry, and the diagonal (column `diag`) and zeros are dropped (setdiag(0); eliminate_zeros(), weightmatrix.py:185-186).
template <class Index>
ASM_FN bool asm_segment(const unsigned long long* key, const double* val, Index e, Index M, int diag, int sym, int* col, double* v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int c = asm_key_col(key[e]);
  *col = c;
  if (e != 0 && asm_key_col(key[e - 1]) == c) return false;
  double a = 0.0, b = 0.0;
  for (Index q = e; q < M && asm_key_col(key[q]) == c; ++q) {
    if (asm_key_kind(key[q])) b = b + val[q]; else a = a + val[q];
  }
  *v = combine_entry(a, b, sym);
  return c != diag && *v != 0.0;
}
