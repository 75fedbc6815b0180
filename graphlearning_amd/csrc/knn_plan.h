// The plan of one pass of the exact kNN search (knn.hip): everything the pass derives from (n, d, k, nq, long_lists, the plan
// overrides) before it touches the device, and the three decisions it takes later from counts the device hands back.  No HIP
// header: tests/test_knn_plan.py builds it on the host and checks the plans of a grid of shapes against a recorded table.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/glx_experimental.h"   // glx_knn_options

static const int BQ = 128;             // queries per workgroup (4 waves x 32)
static const int BR_MAX = 128;         // refs per LDS tile: 32 * NSUB
static const int KBUF = 8;             // per-lane append slots between list merges
static const int KNN_CAT_SEG = 21;     // concatenated split operands: three segments of this many bf16 per row (d <= 21)
static const int FB_SPLIT = 64;        // pieces a fallback row's refs are cut into
static const int FB_CAP = 128;         // candidates per row the one-pass fallback can hold
static const int KNN_K_NARROW = 60;    // neighbours (self included) of the list-returning entry points and of the register re-rank
static const int KNN_K_MAX = 1024;     // neighbours (self included) of the wide search (glx_knn_search)
static const size_t KNN_CAND_BUDGET = (size_t)1 << 30;   // bytes of candidates (value + index) a wide pass holds at once: its query chunks

// ---- the scale of the filter's operands ------------------------------------------------------------------------------------------
// The filter's error bound (cerr, below) is RELATIVE: |filter value - exact dist^2| <= cerr (|q| + rmax)^2 holds while every fp32
// product and sum of the centred operands is a normal number, i.e. loses a relative 2^-24 and not an absolute 2^-149 (or everything:
// overflow).  With rmax the largest centred norm and coordinates c <= rmax:
//   below: a product or a split piece under 2^-126 carries an absolute error <= 2^-126 (flushed altogether at worst); there are
//          3 dpa + 8 products and sums and 2 d pieces per value (d <= 16382), in total U <= 2^-126 (4 sqrt(d) rmax + 2 (3 dpa + 8) + 2 d)
//          <= 2^-108, against a bound of at least cerr rmax^2 >= 2^-16 rmax^2: U is 2^-12 of the bound at rmax = 2^-40;
//   above: filter values reach 4 rmax^2 = 2^82 at rmax = 2^40, far below the 1e30 at which the spare rows behind the data count
//          as infinitely far, and below fp32's 2^128.
// So the bound is valid for KNN_RMAX_LO <= rmax <= KNN_RMAX_HI, and data inside that window is taken as it comes (every list,
// count and statistic of such data is what it was before the window existed).  Outside it the centred operands are multiplied,
// in fp64 and before they are rounded to fp32, by the exact power of two that brings rmax into [1, 2) (knn_rmax_kernel decides,
// on the device; the prep kernels apply it): the filter then works in units of 1 / scale.  Everything in those units stays in
// them -- the norms, rmax itself, eps, the lists' thresholds, the seed --; the two places where a filter value meets an exact fp64
// distance convert: the acceptance test of the re-rank compares with dk2 scale^2, and the seeding pre-pass hands the cell pruning
// ub2 / scale^2.  Measured before the scaling existed (tests/test_gpu_knn_scale.py): wrong lists at data scaled by 2^-72 .. 2^-80
// (values that are multiples of 2^-149 passed the acceptance test) and by 2^+55 (norms of some rows overflow to inf, those refs
// enter no list, and a list that is not full does not count against a row).
// rmax = 0, not finite, or below fp64's normal range: no scaling (nothing would make the filter sharp; the host refuses non-finite
// input, and where the centred norms are subnormal in fp64 the exact distances themselves underflow).
#if defined(__HIPCC__)
#define KNN_HOST_DEVICE __host__ __device__
#else
#define KNN_HOST_DEVICE
#endif
constexpr double KNN_RMAX_LO = 0x1p-40, KNN_RMAX_HI = 0x1p+40;
KNN_HOST_DEVICE inline double knn_filter_scale(double rmax) {
  if (rmax >= KNN_RMAX_LO && rmax <= KNN_RMAX_HI) return 1.0;
  if (!(rmax >= 0x1p-1022 && rmax < 0x1p+1023)) return 1.0;    // 0, subnormal, inf, NaN (and the last binade, whose 2^-E is subnormal)
  uint64_t bits;
  __builtin_memcpy(&bits, &rmax, 8);
  bits = (uint64_t)(2046 - ((bits >> 52) & 0x7ff)) << 52;      // 2^-E for rmax = m 2^E, 1 <= m < 2 (E in [-1022, 1022]: a normal number)
  double scale;
  __builtin_memcpy(&scale, &bits, 8);
  return scale;
}

// ---- the margin of the re-rank's acceptance test -----------------------------------------------------------------------------------
// A row is accepted when every full list's threshold tau satisfies tau >= dk2 + 2 eps: then every ref r the filter rejected (filter
// value >= tau) is at least as far as the k-th candidate (exact squared distance dk2, here in the filter's units).  The filter's error
// on a pair is bounded PER PAIR: every term of the derivation of cerr (knn_make_plan) is a multiple of |q||r|, |q|^2 or |r|^2, so
// |filter - exact| <= E(r) with E(r) < 2 cerr (|q| + |r|)^2, and (|q| + rmax)^2 is only its largest value.  The rejected refs come in
// two kinds.  |r| > |q| + dk: the triangle inequality alone puts r farther than dk, whatever the filter said.  |r| <= R := min(rmax,
// |q| + dk): exact >= tau - E(r) >= tau - 2 cerr (|q| + R)^2.  So eps = cerr (|q| + R)^2 serves, with R taken 2^-10 larger for the
// fp32 norms, plus 2^-12 of the old eps for the absolute errors of underflowing products (knn_filter_scale, above: U is 2^-12 of
// cerr rmax^2 at worst).  For a query far from every ref (dk >= rmax - |q|) this is the old margin cerr (|q| + rmax)^2; for data of
// low intrinsic dimension, where neighbours are close compared with the cloud's radius, it is what keeps the short lists' thresholds
// outside the margin: N(0, 1) data in one dimension, n = 2999, k = 12 sent 1267 rows to the exact fallback with the old margin
// (tests/test_gpu_knn_narrow.py), 4 with this one.
KNN_HOST_DEVICE inline double knn_accept_eps(double cerr, double qnorm, double rmax, double dk2s) {
  const double far = qnorm + rmax;
  const double R = fmin(rmax, (qnorm + sqrt(dk2s)) * (1.0 + 0x1p-10));
  const double near = qnorm + R;
  return cerr * near * near + 0x1p-12 * cerr * far * far;
}

// features per half per block of the blocked (d > 130) fp32 variant; 16 where the KP = 64 lists leave less LDS
constexpr int knn_kb(int KP) { return KP == 64 ? 16 : 32; }   // (KP = 8 never takes the blocked variant)

// fp32-input filter: refs per tile = 32*NSUB, as many as fit LDS (160 KiB) beside the candidate lists
constexpr int tile_nsub(int DH, int KP) {
  const int stride = 2 * DH + 2;
  if (KP == 8) {   // short lists: aim at three workgroups per CU
    for (int ns = 4; ns >= 2; ns /= 2)
      if (2 * 32 * ns * stride * 4 + (KP + KBUF) * 256 * 8 <= 53 * 1024) return ns;
    return 1;
  }
  for (int ns = 4; ns >= 2; ns /= 2)
    if (2 * 32 * ns * stride * 4 + (KP + KBUF) * 256 * 8 <= 78 * 1024) return ns;   // two workgroups per CU
  return 1;
}

// bf16 filter: refs per tile = 32 * NSUB.  Measured (one box): 16-32 features: NSUB 2 (config 2: 1.88 vs 2.12 ms, config 3: 2.74 vs
// 3.09 ms); 64 features: NSUB 1 -- a 17 KB tile lets three workgroups share a CU (n = 1e6: 376 vs 401 ms)
constexpr int bf16_nsub(int NKB, int KP) { return (NKB >= 4 || KP >= 32) ? 1 : 2; }
// 8-entry lists in registers where that buys a fourth workgroup per CU (d = 49 .. 64: 122 registers, 34 KB of LDS; measured
// +4 % at n = 3e5 .. 1e6; at fewer feature blocks the registers spill, at more the kernel is register-bound anyway)
constexpr bool bf16_reglists(int NKB, int KP) { return KP == 8 && NKB == 4; }

struct KnnPlan {
  int KP;               // entries per candidate list
  int DH, nkb;          // fp32-input filter: features per half per block, blocks (1: the query's features stay in registers)
  int NKB;              // bf16 filter: blocks of 16 features (0: the fp32-input filter)
  int dpa;              // padded feature count of the filter's operands
  int BR;               // refs per LDS tile
  int64_t ntiles, nqb;  // ref tiles, query blocks of BQ
  int nsplit, lists;    // ref ranges per query block; lists per query = 2 nsplit
  int ncand, M;         // candidates per query = lists * KP; the re-rank's power of two >= max(64, ncand)
  int64_t chunk, nchunks;   // queries whose candidates are held at once (wide: within KNN_CAND_BUDGET), passes over them
  bool short_lists, wide, use_bf16;
  int cat;              // bf16 filter: 0 blocks of 16 features, 1 concatenated operands, 2 with the norm folded in
  double cerr;          // |filter value - exact dist^2| <= cerr * (|q| + rmax)^2, for operands scaled by knn_filter_scale(rmax)
};

inline KnnPlan knn_make_plan(int64_t n, int d, int k, int64_t nq, bool long_lists, const glx_knn_options& opt) {
  // d + 2 <= 132: the query's features stay in registers; above that the feature dimension is blocked
  int KP = k <= 12 ? 16 : (k <= 28 ? 32 : 64);
  // Short lists.  A query's candidates are kept in 2*nsplit separate lists (two half-wavefronts x
  // nsplit ref ranges); with >= 8 lists, 8 entries per list hold the k <= 12 nearest unless 8 of
  // them fall into the same list (5e-5 per query for k = 11; the acceptance test of the re-rank
  // sees a full list whose threshold is too small and sends the row to the exact fallback).  The
  // shorter lists free LDS for a third workgroup per CU and halve the list rescans: 5.1 -> 3.6 ms
  // at config 2, 94 -> 108 TFLOP/s at d = 64.  Not for the blocked variant: at large d the fp32
  // error margin of the acceptance test makes short lists fall back too often.
  // The same argument one size up: 16 entries for k <= 28 (3e-7 per query at k = 28), 32 for k <= 60.
  const bool short_lists = !long_lists && d + 2 <= 132 && opt.lists != 2;
  if (short_lists) KP = k <= 12 ? 8 : (k <= 28 ? 16 : 32);
  // The wide plan (k > 60): lists of 32 wherever the short lists apply (d + 2 <= 132: the split-bf16 filter for d <= 128, the
  // fp32-input one for d = 129, 130), of 64 (the fp32-input filter) for the long lists and d > 130; ref ranges such that the
  // 2 nsplit lists hold about 4 k candidates (below)
  const bool wide = k > KNN_K_NARROW;
  if (wide) KP = short_lists ? 32 : 64;
  int DH = knn_kb(KP), nkb = 1;
  if (d + 2 <= 132 && !(KP == 64 && d + 2 > 36)) {   // (KP = 64 lists + a wide double-buffered tile exceed the LDS)
    for (int cand : {8, 12, 18, 34, 66})
      if (2 * cand >= d + 2) { DH = cand; break; }
  } else {
    nkb = (d + 2 + 2 * DH - 1) / (2 * DH);
  }
  // Filter arithmetic.  Default: split-bf16 operands on the bf16 matrix cores (d <= 128 with the short lists); the fp32-input
  // MFMA kernel serves everything else (and glx_knn_options::filter = 2).
  const bool use_bf16 = short_lists && d <= 128 && KP <= 32 && opt.filter != 2;
  int NKB = 0;
  if (use_bf16) {
    for (int cand : {1, 2, 4, 6, 8})
      if (16 * cand >= d) { NKB = cand; break; }
  }
  const int dpa = use_bf16 ? 16 * NKB : 2 * DH * nkb;
  const int64_t nqb = (nq + BQ - 1) / BQ;
  const int BR = use_bf16 ? 32 * bf16_nsub(NKB, KP) : 32 * tile_nsub(DH, KP);
  const int64_t ntiles = (n + BR - 1) / BR;
  int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8, ntiles), (1024 + nqb - 1) / nqb));
  if (short_lists) {
    // >= 8 lists per query; 16 for the 8-entry lists once the data no longer sits in cache (an exact
    // fallback row then streams all of X k times: 329 rows cost 0.6 s at n = 2e6 -- with 16 lists 5 rows are left)
    const int64_t want = (KP == 8 && (double)n * d * 8.0 > 64.0 * 1024 * 1024) ? 8 : 4;
    nsplit = (int)std::max<int64_t>(nsplit, std::min<int64_t>(want, ntiles));
  }
  if (opt.nsplit > 0) nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8, ntiles), opt.nsplit));
  if (wide) {
    // 2 nsplit lists of KP, nsplit a power of two in [8, 32] (or the number of ref tiles when there are fewer: n = 257 gives 9):
    // lists * KP >= 4 k where 32 ranges allow it (k <= 128 with 32 entries: 16 lists, 512 candidates; k = 1024 with 64 entries:
    // 64 lists).  A query's k nearest then fill a list to a quarter on average,
    // and the smallest full list's threshold lies well beyond the k-th distance.  Above k = 512 the 64 lists of 32 hold 2 k: half
    // full on average, 1.9 % of config 2's rows go to the fallback at k = 1024 -- and the search takes half the time of the fp32
    // filter's 64 lists of 64 (34 vs 65 ms of kernels, profiles/knn_wide_k.txt).  With fewer tiles than that (n < 32 nsplit)
    // every range is one tile of 32 refs, whose half of 16 fits any list: all refs are candidates.  An override never goes below
    // k candidates.
    int want = 8;
    while (want < 32 && 2 * want * KP < 4 * k) want *= 2;
    if (opt.nsplit > 0) want = std::max(opt.nsplit, (k + 2 * KP - 1) / (2 * KP));
    nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(32, ntiles), want));
  }
  const int lists = nsplit * 2;
  const int ncand = lists * KP;
  int M = 64;
  while (M < ncand) M *= 2;
  // wide: the queries in chunks whose candidates (8 bytes each) stay within a fixed budget -- 2.3 GB at 70 000 rows x 4096
  // candidates otherwise, 33 GB at 10^6; the lists of k <= 60 are short enough to be held for all queries at once
  const int64_t chunk = wide ? std::min<int64_t>(nq, std::max<int64_t>(BQ, (int64_t)((KNN_CAND_BUDGET / ((size_t)ncand * 8)) / BQ * BQ))) : nq;
  const int64_t nchunks = (nq + chunk - 1) / chunk;
  // |filter value - exact dist^2| <= cerr * (|q| + rmax)^2, valid for KNN_RMAX_LO <= rmax <= KNN_RMAX_HI (above: the products and sums
  // of the bound's derivation are normal fp32 numbers there); knn_filter_scale brings every other input into that range.
  // fp32 filter: input rounding (2^-24 per coordinate), dpa products and sums at 2^-24 each, norms computed in fp32; generous constant.
  // bf16 filter: eps = cerr (|q| + rmax)^2 with cerr ~ 2^-16.  The dropped parts of the split products (lo.lo and the residuals of the
  // two roundings) are <= 3.1 * 2^-16 |q||r| in q.r in the worst case -- every coordinate's errors at their bounds and aligned --, twice
  // that in the distance, i.e. <= 1.55 * 2^-16 (|q| + rmax)^2; plus 3 kpad fp32 accumulations, fp32 norms and input rounding (the second
  // term, doubled: the matrix pipe's internal rounding mode is not documented).  So |filter - exact| < 2 eps within that range, which is what the
  // acceptance test of the re-rank needs (it asks for a margin of 2 eps), and <= 0.52 eps on every pair of the randomised suite's inputs
  // (an emulation of the split arithmetic: profiles/r05_knn_tile_pmc.txt); the re-rank's fp32 screen allows for 2 eps per value as well.
  const double cerr = use_bf16 ? 2.0 * (std::ldexp(1.0, -17) + (1.5 * (3.0 * dpa + 4.0) + d + 16.0) * std::ldexp(1.0, -24))
                               : (double)(dpa + 8) * std::ldexp(1.0, -22);
  // 17 <= d <= 21 (two blocks of 16 per half): the three split products as ONE contraction over concatenated operands,
  // 4 MFMAs per 32 x 32 tile instead of 6 (d <= 16 needs 3 either way)
  // ... and for d <= 20 with the norm folded in (glx_knn_options::concat = 1: without the fold, 0: blocks of 16 features)
  int cat = 0;
  if (use_bf16) {
    cat = (d <= KNN_CAT_SEG && NKB == 2) ? (d < KNN_CAT_SEG ? 2 : 1) : 0;
    if (opt.concat >= 0) cat = std::min(cat, opt.concat);
  }
  return {KP, DH, nkb, NKB, dpa, BR, ntiles, nqb, nsplit, lists, ncand, M, chunk, nchunks, short_lists, wide, use_bf16, cat, cerr};
}

// The seeding pre-pass (knn_seed_kernel) runs the tile kernel over a sample of the refs first and starts every list of the
// search proper at a threshold derived from it.  Over all refs it does not pay (measured, profiles/r03_knn_seed.txt: the k-th
// of a 1/8 sample is the 8k-th of the whole set, 79 % of the wave-tiles still hold a candidate and the pre-pass costs its
// eighth); the cell-pruned search needs it: its bound ub2 decides which cells a query block visits.
// ncells: the cells the rows come in (0: none).  sub: the tile stride of the sample (0: no cells).
struct KnnSeedPlan { int sub; bool seeded; };
inline KnnSeedPlan knn_seed_plan(const KnnPlan& p, int k, int ncells) {
  const bool cells = ncells > 1;
  // sample the block's own cells: every tile of small cells, every 8th of cells of >= 128 tiles
  const int seed_sub = cells ? (int)std::max<int64_t>(1, std::min<int64_t>(8, std::max<int64_t>(1, p.ntiles / ncells) / 16)) : 0;
  // (not for the wide plan: its lists hold a fraction of k each, and the search stays all pairs -- on the reordered rows if any)
  const bool seeded = cells && 2 * p.KP >= k && !p.wide;
  return {seed_sub, seeded};
}

// nbad query rows failed the acceptance test of the short lists: repair row by row, or search again with the long lists?
// A fallback row streams the data once (measured: ~5 TB/s);
// the repeat costs about four tile-kernel times (fp32-input filter, longer lists)
// visited_share: the share of the (query block, ref tile) pairs a cell-pruned first pass visited; 1 for all pairs.
inline bool knn_should_escalate(const KnnPlan& p, int64_t n, int d, int k, int64_t nq, size_t nbad, double visited_share) {
  if (!(p.short_lists && p.KP < 64 && nbad > 64)) return false;
  // The first pass is priced by a MODEL, not by its measured time: the choice must not depend on who else uses the GPU (with six
  // processes sharing it the measured pass came out long enough, once in thirty runs, to send 21 000 rows of
  // tests/test_gpu_knn.py::test_search_on_data_sorted_by_locality through the row-by-row repair -- the right answer, the slow way).
  // 1.26e10 (query, ref, 16-feature block) triples per ms: config 2's 0.78 ms for 70 000^2 pairs of two blocks.
  const double share = std::max(visited_share, 0.01);
  // (the fp32-input filter runs at a quarter of that: profiles/r02_knn_filter_probe.txt, d = 64 / 128; 0.03 ms: launches + the host look of a tiny pass)
  const double ms_first = std::max(0.03, (double)nq * (double)n * share * ((double)p.dpa / 16.0) / 1.26e10 * (p.use_bf16 ? 1.0 : 4.0));
  // (one pass per row: knn_fallback_collect_kernel; wide: plus the ranking of about k refs per row, 12 ns each -- measured at
  // config 2, k = 1024: 1332 rows in 19.4 ms)
  const double ms_rows = (double)nbad * ((double)n * d * 8.0 / 5e9 + (p.wide ? 1.2e-5 * k : 0.0));
  // (the wide plan's repeat -- the fp32-input filter with lists of 64 over as many ranges, and the re-rank of up to 4096
  // candidates -- measured 52 and 83 times the model's first pass at config 2, k = 512 and 1024: priced at 60)
  return ms_rows > (p.wide ? 60.0 : 4.0) * ms_first;
}

// the wide fallback of nr flagged rows: the one-pass buffer from k (a power of two >= 2 k), sorted in LDS; rows in batches whose
// k-round buffers stay within 256 MiB
struct KnnWideFallbackPlan { int cap; size_t batch; };
inline KnnWideFallbackPlan knn_wide_fallback_plan(int k, size_t nr) {
  int cap = FB_CAP;
  while (cap < 2 * k) cap *= 2;
  const size_t per_row = (size_t)FB_SPLIT * k * 12 + (size_t)cap * 12 + 8;
  const size_t batch = std::max<size_t>(1, std::min(nr, ((size_t)256 << 20) / per_row));
  return {cap, batch};
}

// the cells in a chain of nearest centres (greedy, from the centre farthest from the centres' mean): neighbouring cells of
// feature space end up next to each other in the row order, which then serves as a locality order for the graph's operators
// too (one XCD's share of the rows = a few whole clusters; with the cells in arbitrary order the sweep at 10^6 rows ran 20 % slower).
// cen: the m centres, d doubles each; returns place[cell] = its position in the chain.
inline std::vector<int> knn_chain_places(const std::vector<double>& cen, int m, int d) {
  std::vector<double> mean(d, 0.0);
  for (int c = 0; c < m; ++c)
    for (int f = 0; f < d; ++f) mean[f] += cen[(size_t)c * d + f] / m;
  const int cfs = (d + 31) / 32;       // (every cfs-th feature, as in the assignment: m^2 d flops on one host thread otherwise)
  auto dist2 = [&](const double* a, const double* bb) { double t = 0; for (int f = 0; f < d; f += cfs) { const double q = a[f] - bb[f]; t += q * q; } return t; };
  int cur = 0;
  double far = -1.0;
  for (int c = 0; c < m; ++c) { const double t = dist2(&cen[(size_t)c * d], mean.data()); if (t > far) { far = t; cur = c; } }
  std::vector<int> place(m, -1);
  for (int pos = 0; pos < m; ++pos) {
    place[cur] = pos;
    int nxt = -1;
    double best = INFINITY;
    for (int c = 0; c < m; ++c)
      if (place[c] < 0) { const double t = dist2(&cen[(size_t)c * d], &cen[(size_t)cur * d]); if (t < best) { best = t; nxt = c; } }
    if (nxt < 0) break;
    cur = nxt;
  }
  return place;
}
