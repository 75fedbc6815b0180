// The host arithmetic of the two conjugate-gradient solves (cg.hip reference-order, cg_fused.hip tolerance mode): limits, numpy's
// pairwise-summation tree, the per-system stop state, chunk lengths, reduction forms, the staged upload, the replay key.
// No HIP header: tests/cg_plan_host.cpp builds it with plain g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../include/glx.h"   // the GLX_* codes and the GLX_CG_* flags

// ---- limits: what each mode refuses (the code, and the message in `msg`) ---------------------------------------------------------
struct CgShape {
  int64_t n;            // rows
  int C, Cg;            // columns, columns per system
  int ncols, ld;        // columns padded to the 4-wide vectors, elements per record
  int64_t max_iter;
  int ngroups;          // systems
  int64_t nmask;        // Dirichlet rows of all systems
};
#define CG_LIMIT(cond, ...) do { if (!(cond)) { snprintf(msg, cap, __VA_ARGS__); return GLX_EUNSUPPORTED; } } while (0)
inline int cg_exact_limits(const CgShape& s, char* msg, size_t cap) {
  CG_LIMIT(s.ncols <= 256, "glx_cg_multi: C=%d too wide for the column reducer", s.C);
  CG_LIMIT(s.Cg <= 128, "glx_cg_multi: %d columns per system too wide for the reference-order reducer", s.Cg);
  CG_LIMIT(256 / (s.ld / 4) >= 1, "glx_cg_multi: record too wide");
  CG_LIMIT(s.max_iter < (1ll << 24), "glx_cg_multi: max_iter %lld exceeds the supported 2^24-1", (long long)s.max_iter);
  CG_LIMIT(s.n < (1ll << 27), "glx_cg_multi: %lld rows exceed the reference-order reducer's 32-bit offsets", (long long)s.n);
  return GLX_OK;
}
inline int cg_fused_limits(const CgShape& s, char* msg, size_t cap) {
  CG_LIMIT(s.ncols <= 256, "glx_cg_multi: C=%d too wide for the column reducer", s.C);
  CG_LIMIT(256 / (s.ld / 4) >= 1, "glx_cg_multi: record too wide");
  CG_LIMIT(s.max_iter < (1ll << 24), "glx_cg_multi: max_iter %lld exceeds the supported 2^24-1", (long long)s.max_iter);
  CG_LIMIT(s.nmask == 0 || s.ngroups <= 32,
           "glx_cg_groups_masked: at most 32 systems with Dirichlet rows per tolerance-mode solve (got %d)", s.ngroups);
  return GLX_OK;
}
#undef CG_LIMIT

// ---- numpy's pairwise summation: the recursion of DOUBLE_pairwise_sum on (offset, n) ---------------------------------------------
struct PwHost {
  std::vector<int64_t> leaf_off;
  std::vector<int32_t> leaf_len, node_l, node_r, node_h, level_start;
  // returns a provisional id: leaves >= 0, internal nodes as -(index + 1)
  int build(int64_t off, int64_t n, int* height) {
    if (n <= 128) {
      leaf_off.push_back(off);
      leaf_len.push_back((int32_t)n);
      *height = 0;
      return (int)leaf_off.size() - 1;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    int hl, hr;
    const int l = build(off, n2, &hl);
    const int r = build(off + n2, n - n2, &hr);
    *height = std::max(hl, hr) + 1;
    node_l.push_back(l);
    node_r.push_back(r);
    node_h.push_back(*height);
    return -(int)node_l.size();
  }
  // numpy hands a contiguous 1-D reduction to the pairwise routine in pieces of its buffer size
  // (8192 elements) and adds the pieces' sums one after another: ((c0 + c1) + c2) + ...
  void build_chunked(int64_t n) {
    const int64_t NPY_BUFSIZE = 8192;
    int h, hacc = 0;
    int acc = build(0, std::min(n, NPY_BUFSIZE), &hacc);
    for (int64_t off = NPY_BUFSIZE; off < n; off += NPY_BUFSIZE) {
      const int c = build(off, std::min(NPY_BUFSIZE, n - off), &h);
      hacc = std::max(hacc, h) + 1;
      node_l.push_back(acc);
      node_r.push_back(c);
      node_h.push_back(hacc);
      acc = -(int)node_l.size();
    }
  }
  void finish() {   // order the internal nodes by height (stable: children always precede parents) and renumber
    const int ni = (int)node_l.size(), nl = (int)leaf_off.size();
    std::vector<int> order(ni);
    for (int q = 0; q < ni; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return node_h[x] < node_h[y]; });
    std::vector<int> newpos(ni);
    for (int q = 0; q < ni; ++q) newpos[order[q]] = q;
    auto remap = [&](int id) { return id >= 0 ? id : nl + newpos[-id - 1]; };
    std::vector<int32_t> l2(ni), r2(ni);
    int maxh = 0;
    for (int q = 0; q < ni; ++q) {
      l2[q] = remap(node_l[order[q]]);
      r2[q] = remap(node_r[order[q]]);
      maxh = std::max(maxh, (int)node_h[order[q]]);
    }
    level_start.assign(maxh + 1, 0);
    for (int q = 0; q < ni; ++q) level_start[node_h[order[q]]]++;   // counts per height h >= 1 at index h
    // prefix: level_start[h-1] = first internal node of height h
    std::vector<int32_t> ls(maxh + 1, 0);
    int acc = 0;
    for (int h = 1; h <= maxh; ++h) { ls[h - 1] = acc; acc += level_start[h]; }
    ls[maxh] = acc;
    level_start = ls;
    node_l = l2;
    node_r = r2;
  }
};

// ---- stop state: which systems stopped where, as the rows of the residual history arrive ------------------------------------------
struct CgStop {
  int ngroups, stride;
  double tol;
  std::vector<int64_t> iters;       // iterations that ran, per system (utils.py:522 `i`)
  std::vector<double> err;          // utils.py:519
  std::vector<char> done;
  int running = 0;
  double e_prev = 1.0, e_last = 1.0;   // the two latest maxima over the running systems the host has seen
  double margin_seen = INFINITY;       // min over every decision taken of |err - tol| / tol (glx_cg_last_stop_margin)
  CgStop(int ngroups_, double tol_)
      : ngroups(ngroups_), stride(ngroups_ + 1), tol(tol_), iters(ngroups_, 0), err(ngroups_, 1.0), done(ngroups_, !(1.0 > tol_)) {
    for (int g = 0; g < ngroups; ++g) running += !done[g];
  }
  // rows [it0 + 1, it0 + cnt] of the residual history have arrived in `h`
  void read(const double* h, int64_t it0, int64_t cnt) {
    for (int64_t q = 0; q < cnt && running > 0; ++q) {
      // iteration it0+q+1 ran for every system whose previous err was > tol; its err decides the next one
      for (int g = 0; g < ngroups; ++g) {
        if (done[g]) continue;
        iters[g] = it0 + q + 1;
        err[g] = h[(size_t)q * stride + g];
        // EVERY residual norm a running system shows is a stop decision (CG's residual norms are not monotone: one that came within
        // the band of tol on the far side iterations ago could have stopped the reference's order of additions there)
        if (tol > 0 && err[g] == err[g]) margin_seen = std::min(margin_seen, fabs(err[g] - tol) / tol);
        if (!(err[g] > tol)) { done[g] = 1; --running; }   // (a NaN stops its own system)
      }
      e_prev = e_last;
      e_last = h[(size_t)q * stride + ngroups];
    }
  }
};

// ---- tolerance mode: iterations per captured chunk --------------------------------------------------------------------------------
// Every hand-over from one launched graph to the next costs ~37 us of idle device (kernel trace: profiles/r04_cg_tree_chunks.txt)
// whether or not the next one was enqueued in time, an iteration past convergence ~9 us (its two kernels exit at once): long chunks
// while the end is far, short ones near it.
static const int CG_NLEN = 3;
static const int CG_LEN[CG_NLEN] = {32, 16, 4};
static const int CG_LONG = 32;                 // (the longest: sizes the history buffers)
// CG's error falls roughly geometrically, the last ratio predicts the iterations still needed, and the longest chunk that does not
// overshoot them by more than two is launched
inline int cg_next_kind(int64_t looked, int64_t launched, double e_prev, double e_last, double tol) {
  if (looked < 4) return CG_NLEN - 1;                           // nothing seen yet: the short chunk behind the first one
  if (!(e_last > tol) || !(e_last < e_prev)) return 1;
  const double rate = e_last / e_prev;
  const double need = log(tol / e_last) / log(rate);           // iterations still needed after `looked`
  const double open = need - (double)(launched - looked);      // ... of which not yet launched
  for (int v = 0; v < CG_NLEN - 1; ++v)
    if ((double)CG_LEN[v] <= open + 2.0) return v;
  return CG_NLEN - 1;
}

// ---- reference-order mode: the form of the two reduction chains -------------------------------------------------------------------
static const int CG_CHUNK = 8;
// the chains are walked row by row (cg_seqsum_dpp_kernel, 2.4 ns per row) or in block form (cg_seqsum.hip: integer block sums
// confirmed by the exact state; same bits) -- the block form from 8192 rows on
inline bool cg_first_blocks(int64_t n, int flags, bool np1d, int nchunks, int max_chunks, size_t rec_bytes) {
  return !np1d && !(flags & GLX_CG_CHAIN) && nchunks <= max_chunks && n >= 1 &&
         rec_bytes <= ((size_t)1 << 30) &&      // (hundreds of columns x millions of rows: the chain)
         ((flags & GLX_CG_BLOCKS) || n >= 8192);
}
// Per kind of reduction (0: p.Ap, 1: r.r) the form is re-decided whenever the host looks at the residual history: the block
// form costs about a microsecond per block that is not a plain same-binade one (a lone wavefront issues an instruction every
// four cycles), the chain 2.4 ns per row -- products that cancel (the singular Poisson system on separate clusters: p.Ap
// changes sign from row to row) are cheaper row by row.  Same bits either way, so switching in mid-solve changes nothing but time.
struct CgForms {
  bool blocks_now[2];
  bool adaptive;        // block form, and not forced (GLX_CG_BLOCKS)
  // A chunk launched ahead runs in the forms decided one look earlier.  While a kind of reduction in block form is anywhere near the price
  // of the chain (products that cancel: its walk can cost twice the chain), a late switch costs more than the bubble of waiting for the
  // look: one chunk in flight until the block form has shown itself cheap (under half the chain) or is no longer in use.
  bool ahead;
  unsigned long long ss_seen[2][3] = {{0, 0, 0}, {0, 0, 0}};
  CgForms(bool ss_blocks, bool forced) : blocks_now{ss_blocks, ss_blocks}, adaptive(ss_blocks && !forced), ahead(!adaptive) {}
  // `hs`: the counters [kind][4] (blocks taken plain / by record / row by row) as a chunk of `cnt` iterations left them
  void look(const unsigned long long* hs, int cnt, int ncols, int64_t n, int nchunks) {
    if (!adaptive) return;
    bool cheap = true;
    for (int m = 0; m < 2; ++m) {
      if (!blocks_now[m]) continue;
      const double by_rec = (double)(hs[4 * m + 1] - ss_seen[m][1]), by_rows = (double)(hs[4 * m + 2] - ss_seen[m][2]);
      for (int q = 0; q < 3; ++q) ss_seen[m][q] = hs[4 * m + q];
      const double chains = (double)cnt * ncols;
      // measured on one MI355X (profiles/r06_cg_blocks_kernel_stats.csv): 0.7 us per block taken through its record, 1.5 per 256-row
      // block taken row by row (0.65 of additions -- the chain's 2.4 ns per row --, the rest its rows arriving: three are fetched
      // ahead per chunk; 399 us for a walk with every one of its 274 blocks row by row), 0.6 per chunk of the walk, 14.5 for the two
      // passes in front; the chain 2.4 ns per row
      const double blocks_us = (by_rec * 0.7 + by_rows * 1.5) / chains + nchunks * 0.6 + 14.5;
      const double chain_us = (double)n * 0.0024;
      if (blocks_us > chain_us) blocks_now[m] = false;
      else if (blocks_us > 0.5 * chain_us) cheap = false;
    }
    ahead = cheap;
  }
};

// ---- tolerance mode: the one staged upload [right-hand side rows | Dirichlet rows | their systems | values | output scale] ---------
struct CgStage { size_t rows, mrows, mgrp, vals, scale, bytes; };
// nb rows of C values of esize bytes (0: a dense right-hand side), nmask Dirichlet rows, nscale doubles of output scale (0: none)
inline CgStage cg_stage_layout(int64_t nb, int64_t nmask, int C, size_t esize, int64_t nscale) {
  CgStage s;
  s.rows = 0;
  s.mrows = s.rows + (size_t)nb * 4;
  s.mgrp = s.mrows + (size_t)nmask * 4;
  s.vals = (s.mgrp + (size_t)nmask * 4 + 15) / 16 * 16;
  s.scale = (s.vals + (size_t)nb * C * esize + 15) / 16 * 16;
  s.bytes = s.scale + (size_t)nscale * 8;
  return s;
}

// ---- replay key: everything a captured launch sequence was given (a replay is only valid for the same arguments) -------------------
inline unsigned long long cg_key_word(const void* p) { return (unsigned long long)(uintptr_t)p; }
inline unsigned long long cg_key_word(double d) { unsigned long long w; memcpy(&w, &d, 8); return w; }
template <class I> typename std::enable_if<std::is_integral<I>::value, unsigned long long>::type cg_key_word(I i) { return (unsigned long long)i; }
template <class... A> std::vector<unsigned long long> cg_replay_key(const A&... a) { return {cg_key_word(a)...}; }
