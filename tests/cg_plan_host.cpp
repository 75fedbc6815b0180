// Host driver of graphlearning_amd/csrc/cg_plan.h for tests/test_cg_plan_host.py (no HIP header on the include path).
//   pw N             numpy's pairwise-summation tree for N elements: "nleaves ninternal nlevels", then one "off len" per leaf, then one
//                    "level left right" per internal node in value order (value index space: leaves, then internal nodes by level)
//   stop FILE NG TOL CHUNK ROWS   CgStop over the history in FILE (rows of NG + 1 doubles), read CHUNK rows at a time up to ROWS rows:
//                    "running e_prev e_last margin", then "iters err done" per system (doubles as hex floats)
//   plans            the recorded decisions (tests/golden/cg_plans.txt): K rows (chunk length of the tolerance mode), F rows (reduction
//                    forms of the reference-order mode over two looks), D rows (its first decision), L rows (limits)
//   stage            one row per case of the staged upload's grid: "nb nmask C esize nscale | rows mrows mgrp vals scale bytes"
//   key              cg_replay_key of a pointer, an int, an int64, a bool and a double: the words in hex
#include "cg_plan.h"
#include <cstdlib>

// ---- what the rows of `plans` evaluate --------------------------------------------------------------------------------------------
static int eval_kind(int64_t looked, int64_t launched, double e_prev, double e_last, double tol) {
  return cg_next_kind(looked, launched, e_prev, e_last, tol);
}
struct EvalForms {
  CgForms f;
  int64_t n;
  int ncols, nchunks;
  EvalForms(bool ss_blocks, bool forced, int64_t n_, int ncols_, int nchunks_) : f(ss_blocks, forced), n(n_), ncols(ncols_), nchunks(nchunks_) {}
  void look(const unsigned long long* hs, int cnt) { f.look(hs, cnt, ncols, n, nchunks); }
  void print() const {
    printf(" | %d %d %d", (int)f.blocks_now[0], (int)f.blocks_now[1], (int)f.ahead);
    for (int m = 0; m < 2; ++m)
      for (int q = 0; q < 3; ++q) printf(" %llu", f.ss_seen[m][q]);
  }
};
static bool eval_first(int64_t n, int flags, bool np1d, int nchunks, int max_chunks, size_t rec_bytes) {
  return cg_first_blocks(n, flags, np1d, nchunks, max_chunks, rec_bytes);
}
static int eval_limit(int mode, const CgShape& s, char* msg, size_t cap) {
  return mode == 0 ? cg_exact_limits(s, msg, cap) : cg_fused_limits(s, msg, cap);
}

// ---- the grids --------------------------------------------------------------------------------------------------------------------
static void kind_rows() {
  const double tol = 1e-9, nan = std::nan("");
  for (int64_t looked : {0, 3, 4, 20})
    for (int64_t ahead : {0, 4, 16, 32, 48}) {
      for (double ratio : {0.1, 0.5, 0.9, 0.999, 1.0, 1.5})
        for (double over : {0.5, 1.0, 2.0, 1e3, 1e9}) {
          const double e_last = over * tol, e_prev = e_last / ratio;
          printf("K %lld %lld %a %a %a | %d\n", (long long)looked, (long long)(looked + ahead), e_prev, e_last, tol,
                 eval_kind(looked, looked + ahead, e_prev, e_last, tol));
        }
      printf("K %lld %lld nan %a %a | %d\n", (long long)looked, (long long)(looked + ahead), 1e-3, tol, eval_kind(looked, looked + ahead, nan, 1e-3, tol));
      printf("K %lld %lld %a nan %a | %d\n", (long long)looked, (long long)(looked + ahead), 1e-3, tol, eval_kind(looked, looked + ahead, 1e-3, nan, tol));
    }
}

// two looks: counters after a chunk in which every chain took r0 (p.Ap) / r1 (r.r) blocks row by row and 5 through their record, then
// after a chunk of plain blocks only -- a kind that left the block form at the first look is skipped at the second
static void forms_rows() {
  const int rs[] = {0, 2, 10, 40, 60, 200, 1000, 2000};
  for (int64_t n : {(int64_t)8192, (int64_t)70000, (int64_t)1000000})
    for (int ncols : {4, 12, 256})
      for (int cnt : {1, 8})
        for (int forced = 0; forced < 2; ++forced)
          for (int r0 : rs)
            for (int r1 : rs) {
              if (forced && (r0 != 2000 || r1 != 0)) continue;
              const unsigned long long chains = (unsigned long long)cnt * ncols;
              EvalForms e(true, forced != 0, n, ncols, (int)((n + 16383) / 16384));
              unsigned long long hs[16] = {0};
              const int r[2] = {r0, r1};
              for (int m = 0; m < 2; ++m) {
                hs[4 * m + 0] = 100 * chains;
                hs[4 * m + 1] = 5 * chains;
                hs[4 * m + 2] = r[m] * chains;
              }
              printf("F %lld %d %d %d %d %d", (long long)n, ncols, cnt, forced, r0, r1);
              e.look(hs, cnt);
              e.print();
              for (int m = 0; m < 2; ++m) hs[4 * m + 0] += 7 * chains;
              e.look(hs, cnt);
              e.print();
              printf("\n");
            }
  EvalForms chain(false, false, 70000, 12, 5);      // the chain form from the start: nothing to decide, chunks launched ahead
  const unsigned long long hs[16] = {1, 2, 3, 0, 4, 5, 6, 0};
  printf("F 70000 12 8 chain");
  chain.look(hs, 8);
  chain.print();
  printf("\n");
}

static void first_rows() {
  const int max_chunks = 64;
  for (int64_t n : {0, 1, 8191, 8192})
    for (int flags : {0, GLX_CG_CHAIN, GLX_CG_BLOCKS, GLX_CG_NP1D, GLX_CG_CHAIN | GLX_CG_BLOCKS})
      for (int np1d = 0; np1d < 2; ++np1d)
        for (int nchunks : {1, max_chunks, max_chunks + 1})
          for (size_t rec : {(size_t)1000, (size_t)1 << 30, ((size_t)1 << 30) + 1})
            printf("D %lld %d %d %d %d %zu | %d\n", (long long)n, flags, np1d, nchunks, max_chunks, rec,
                   (int)eval_first(n, flags, np1d != 0, nchunks, max_chunks, rec));
}

static void limit_rows() {
  //                         n      C   Cg  ncols ld  max_iter ngroups nmask
  const CgShape ok = {1000, 4, 4, 4, 4, 100, 1, 0};
  std::vector<CgShape> cases = {ok};
  auto with = [&](auto change) { CgShape s = ok; change(s); cases.push_back(s); };
  with([](CgShape& s) { s.C = 256; s.Cg = 128; s.ngroups = 2; s.ncols = 256; s.ld = 256; });
  with([](CgShape& s) { s.C = 257; s.Cg = 1; s.ngroups = 257; s.ncols = 260; s.ld = 260; });
  with([](CgShape& s) { s.C = s.Cg = s.ncols = s.ld = 128; });
  with([](CgShape& s) { s.C = s.Cg = 129; s.ncols = s.ld = 132; });
  with([](CgShape& s) { s.max_iter = (1ll << 24) - 1; });
  with([](CgShape& s) { s.max_iter = 1ll << 24; });
  with([](CgShape& s) { s.n = (1ll << 27) - 1; });
  with([](CgShape& s) { s.n = 1ll << 27; });
  with([](CgShape& s) { s.C = s.ngroups = 32; s.Cg = 1; s.ncols = s.ld = 32; s.nmask = 5; });
  with([](CgShape& s) { s.C = s.ngroups = 33; s.Cg = 1; s.ncols = s.ld = 36; s.nmask = 5; });
  with([](CgShape& s) { s.C = s.ngroups = 33; s.Cg = 1; s.ncols = s.ld = 36; s.nmask = 0; });
  with([](CgShape& s) { s.ld = 1024; });
  with([](CgShape& s) { s.ld = 1028; });
  for (int mode = 0; mode < 2; ++mode)
    for (const CgShape& s : cases) {
      char msg[192] = "";
      const int rc = eval_limit(mode, s, msg, sizeof msg);
      printf("L %d %lld %d %d %d %d %lld %d %lld | %d | %s\n", mode, (long long)s.n, s.C, s.Cg, s.ncols, s.ld, (long long)s.max_iter, s.ngroups,
             (long long)s.nmask, rc, msg);
    }
}

static void plans() {
  kind_rows();
  forms_rows();
  first_rows();
  limit_rows();
}
// ---- end of the recorded part ------------------------------------------------------------------------------------------------------

static int pw(int64_t n) {
  PwHost ph;
  ph.build_chunked(n);
  ph.finish();
  const size_t nl = ph.leaf_off.size(), ni = ph.node_l.size();
  const int nlevels = ph.level_start.empty() ? 0 : (int)ph.level_start.size() - 1;
  printf("%zu %zu %d\n", nl, ni, nlevels);
  for (size_t q = 0; q < nl; ++q) printf("%lld %d\n", (long long)ph.leaf_off[q], ph.leaf_len[q]);
  for (int h = 0; h < nlevels; ++h)
    for (int q = ph.level_start[h]; q < ph.level_start[h + 1]; ++q) printf("%d %d %d\n", h + 1, ph.node_l[q], ph.node_r[q]);
  return ni == 0 || ph.level_start[nlevels] == (int)ni ? 0 : 1;
}

static int stop(const char* path, int ng, double tol, int64_t chunk, int64_t rows) {
  std::vector<double> h((size_t)rows * (ng + 1));
  FILE* f = fopen(path, "rb");
  if (!f || fread(h.data(), 8, h.size(), f) != h.size()) return 1;
  fclose(f);
  CgStop s(ng, tol);
  for (int64_t it0 = 0; it0 < rows; it0 += chunk) s.read(h.data() + (size_t)it0 * (ng + 1), it0, std::min(chunk, rows - it0));
  printf("%d %a %a %a\n", s.running, s.e_prev, s.e_last, s.margin_seen);
  for (int g = 0; g < ng; ++g) printf("%lld %a %d\n", (long long)s.iters[g], s.err[g], (int)s.done[g]);
  return 0;
}

static void stage() {
  for (int64_t nb : {0, 1, 5})
    for (int64_t nmask : {0, 1, 7})
      for (int C : {1, 3, 10})
        for (size_t esize : {(size_t)4, (size_t)8})
          for (int64_t nscale : {0, 11}) {
            const CgStage s = cg_stage_layout(nb, nmask, C, esize, nscale);
            printf("%lld %lld %d %zu %lld | %zu %zu %zu %zu %zu %zu\n", (long long)nb, (long long)nmask, C, esize, (long long)nscale, s.rows, s.mrows,
                   s.mgrp, s.vals, s.scale, s.bytes);
          }
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "pw")) return pw(atoll(argv[2]));
  if (argc == 7 && !strcmp(argv[1], "stop")) return stop(argv[2], atoi(argv[3]), strtod(argv[4], nullptr), atoll(argv[5]), atoll(argv[6]));
  if (argc == 2 && !strcmp(argv[1], "plans")) { plans(); return 0; }
  if (argc == 2 && !strcmp(argv[1], "stage")) { stage(); return 0; }
  if (argc == 2 && !strcmp(argv[1], "key")) {
    const double d = -0.0;
    for (unsigned long long w : cg_replay_key((const int*)0x1234, -1, (int64_t)1 << 40, true, d, 1.5)) printf("%llx\n", w);
    return 0;
  }
  fprintf(stderr, "usage: cg_plan_host pw N | stop FILE NG TOL CHUNK ROWS | plans | stage | key\n");
  return 2;
}
